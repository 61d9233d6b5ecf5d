"""The tracker's call arena on the host (amc-slam_amd/csrc/lba_arena.hpp built alone with g++, tests/native/
arena_harness.cpp): typed sections at 256-byte offsets, the plan's upload and download ranges, its order rule and the
2 GB report.

The expected offsets of the four pinned entry points are literals: the layouts lba_sim3_optimize, lba_sim3_ransac,
lba_triangulate and lba_match_project wrote out by hand before the plan existed (a run of take(n * sizeof(T)) with
out0 and out1 marked between them), worked out for one fixed set of counts each."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN, OUT, WORK = 0, 1, 2
_u64p = ctypes.POINTER(ctypes.c_ulonglong)
_ip = ctypes.POINTER(ctypes.c_int)


@pytest.fixture(scope="module")
def arena():
    src = os.path.join(ROOT, "tests", "native", "arena_harness.cpp")
    out = os.path.join(ROOT, "tests", "native", "_build", "libarena_harness.so")
    deps = [src, os.path.join(ROOT, "amc-slam_amd", "csrc", "lba_arena.hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", src, "-o", out])
    L = ctypes.CDLL(out)
    L.arena_plan.argtypes = [ctypes.c_int, _ip, _ip, _u64p, _u64p, _u64p]
    L.arena_at.argtypes = [ctypes.c_ulonglong] * 2
    L.arena_at.restype = ctypes.c_longlong
    L.arena_image.argtypes = [_ip, ctypes.c_int, _ip, ctypes.c_int, ctypes.c_int, _u64p]
    return L


def plan(L, secs):
    """secs: (kind, element size, count).  Returns (offsets, up_end, down_end, total, misordered, over_2gb)."""
    kind = np.array([s[0] for s in secs], np.int32)
    elem = np.array([s[1] for s in secs], np.int32)
    count = np.array([s[2] for s in secs], np.uint64)
    off, ends = np.zeros(len(secs), np.uint64), np.zeros(3, np.uint64)
    rc = L.arena_plan(len(secs), kind.ctypes.data_as(_ip), elem.ctypes.data_as(_ip), count.ctypes.data_as(_u64p),
                      off.ctypes.data_as(_u64p), ends.ctypes.data_as(_u64p))
    assert rc >= 0
    return [int(o) for o in off], int(ends[0]), int(ends[1]), int(ends[2]), bool(rc & 1), bool(rc & 2)


# (kind, sizeof, count) per section in the entry point's order, then the hand layout's offsets, out0, out1, total
HAND = {
    # 3 pairs, 70 rows, 24 camera rows: S3Pair 96, lba_sim3_corr 112, lba_sim3_cam 88; state, info, flag
    "sim3": ([(IN, 96, 3), (IN, 112, 70), (IN, 88, 24), (OUT, 8, 24), (OUT, 4, 12), (OUT, 4, 70)],
             [0, 512, 8448, 10752, 11008, 11264], 10752, 11776, 11776),
    # 2 pairs, 149 rows, 16 camera rows, 80 hypotheses, 200 mask words: S3RPair 40, lba_s3r_corr 80
    "sim3_ransac": ([(IN, 40, 2), (IN, 80, 149), (IN, 88, 16), (IN, 4, 240), (IN, 4, 80), (OUT, 8, 640), (OUT, 4, 80),
                     (OUT, 4, 80), (OUT, 8, 16), (OUT, 4, 8), (OUT, 4, 149), (WORK, 8, 200)],
                    [0, 256, 12288, 13824, 14848, 15360, 20480, 20992, 21504, 21760, 22016, 22784], 15360, 22784, 24576),
    # 2 chunks, 2 keyframes, 8 camera rows, 70 rows: TriChunk 16, lba_tri_kf 120, lba_tri_cam 168; 16 fields per row
    "triangulate": ([(IN, 16, 2), (IN, 120, 2), (IN, 168, 8), (IN, 4, 140), (IN, 8, 1120), (OUT, 4, 70), (OUT, 4, 70),
                     (OUT, 8, 210)],
                    [0, 256, 512, 2048, 2816, 11776, 12288, 12800], 11776, 14592, 14592),
    # 2 searches, 3 cameras, 9218 cell starts, 90 cell features, 92 features, 58 jobs, 3 camera records, then n_cand
    # and, once the image is filled, 1000 candidates: search 40, cam 20, feat 64, job 96, MatchCamRec 24
    "match": ([(IN, 40, 2), (IN, 20, 3), (IN, 4, 9218), (IN, 4, 90), (IN, 64, 92), (IN, 96, 58), (IN, 4, 58), (IN, 4, 92),
               (IN, 4, 59), (IN, 24, 3), (IN, 4, 58), (IN, 4, 92), (OUT, 4, 232), (OUT, 4, 92), (OUT, 4, 3), (WORK, 4, 58),
               (WORK, 4, 1000)],
              [0, 256, 512, 37632, 38144, 44032, 49664, 49920, 50432, 50688, 50944, 51200, 51712, 52736, 53248, 53504,
               53760], 51712, 53504, 57856),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_the_plan_gives_the_hand_layout(arena, name):
    secs, want_off, out0, out1, total = HAND[name]
    off, up_end, down_end, tot, misordered, over = plan(arena, secs)
    assert off == want_off and (up_end, down_end, tot) == (out0, out1, total)
    assert not misordered and not over
    # every section at a multiple of 256, none overlapping the next, all inside the total
    assert all(o % 256 == 0 for o in off)
    ends = [o + e * c for o, (_, e, c) in zip(off, secs)]
    assert all(e <= nxt for e, nxt in zip(ends, off[1:] + [tot]))
    # the ranges split the sections by kind
    kinds = [k for k, _, _ in secs]
    assert all((o < up_end) == (k == IN) and (o < down_end) == (k != WORK) for o, k in zip(off, kinds))


def test_a_late_work_section_lands_behind_everything(arena):
    secs = HAND["match"][0]
    early = plan(arena, secs[:-1])
    late = plan(arena, secs)
    assert late[0][:-1] == early[0] and late[0][-1] == early[3]         # at the earlier total
    assert late[1:3] == early[1:3] and late[3] == early[3] + 4096       # the ranges stay; 4000 bytes round to 4096


def test_an_empty_section_takes_no_space(arena):
    off, up_end, down_end, total, _, _ = plan(arena, [(IN, 8, 1), (IN, 112, 0), (IN, 4, 1), (OUT, 4, 0), (WORK, 8, 0)])
    assert off == [0, 256, 256, 512, 512] and (up_end, down_end, total) == (512, 512, 512)
    assert plan(arena, [])[1:4] == (0, 0, 0)
    assert plan(arena, [(IN, 4, 64), (IN, 4, 65)])[0] == [0, 256]       # 256 bytes exactly fill their slot
    assert plan(arena, [(IN, 4, 65), (IN, 4, 1)])[0] == [0, 512]


@pytest.mark.parametrize("kinds", [(OUT, IN), (WORK, IN), (WORK, OUT), (IN, OUT, WORK, OUT), (IN, OUT, IN, WORK)])
def test_a_forbidden_order_is_rejected(arena, kinds):
    assert plan(arena, [(k, 4, 10) for k in kinds])[4]


@pytest.mark.parametrize("kinds", [(IN, OUT, WORK), (IN, IN, OUT, OUT, WORK, WORK), (OUT, WORK), (IN, WORK), (WORK,), (OUT,)])
def test_an_allowed_order_is_not(arena, kinds):
    assert not plan(arena, [(k, 4, 10) for k in kinds])[4]


def test_a_total_above_2_gb_is_reported(arena):
    """the limit of lba_sim3_ransac, lba_triangulate and lba_match_project: total > 2^31, whichever kind crosses it"""
    at = [(IN, 8, 1 << 27), (OUT, 8, 1 << 27)]                          # 2^31 exactly: allowed
    assert plan(arena, at)[3] == 1 << 31 and not plan(arena, at)[5]
    for kind in (OUT, WORK):
        total, over = plan(arena, at + [(kind, 4, 1)])[3::2]
        assert total == (1 << 31) + 256 and over
    assert plan(arena, [(IN, 168, 1 << 24)])[5]                         # one section alone
    assert not plan(arena, [(IN, 64, (1 << 25) - 4), (WORK, 4, 64)])[5]   # 2^31 again


def test_the_accessor_adds_the_offset_to_its_base(arena):
    assert arena.arena_at(0, 0) == 0 and arena.arena_at(768, 0) == 768
    assert arena.arena_at(768, 512) == 256                              # a base that is the arena from byte 512 on


def test_the_image_holds_what_was_put(arena):
    a, b = np.arange(70, dtype=np.int32), np.arange(5, dtype=np.int32) + 1000
    offs = np.zeros(5, np.uint64)
    ok = arena.arena_image(a.ctypes.data_as(_ip), 70, b.ctypes.data_as(_ip), 5, 3, offs.ctypes.data_as(_u64p))
    assert ok == 1 and offs.tolist() == [0, 512, 768, 768, 1024]
    ok = arena.arena_image(a.ctypes.data_as(_ip), 0, b.ctypes.data_as(_ip), 5, 0, offs.ctypes.data_as(_u64p))
    assert ok == 1 and offs.tolist() == [0, 0, 256, 256, 256]
