"""The host-side launch plan of the implicit GEMM (csrc/igemm_plan.h) through its query export ``mofa_igemm_plan``, without a GPU:

  (a) every row of tests/igemm_plan_table.json -- the decisions of the commit before the planner existed, see
      tools/igemm_plan_table.py -- is reproduced: tile and split row by row, every field through the table's digests;
  (b) each rule of the planner on the smallest shape that shows it;
  (c) the plan's verdict on invalid arguments is what mofa_igemm_f16 itself returns (NULL stream, nothing can launch);
  (d) the planner is host code: it compiles on its own with g++."""
import ctypes
import json
import os
import shutil
import subprocess

import pytest

import conv_cases as cc
from conv_cases import plan_table as T
from mofa_video_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
T128, T192, T256, T320 = L.TILE_128X128, L.TILE_192X128, L.TILE_256X256, L.TILE_256X320


def plan(a, n_cu=256):
    p = L.IgemmPlan()
    assert L.load().mofa_igemm_plan(ctypes.byref(a), n_cu, ctypes.byref(p)) == 0
    return p


def but(a, **fields):
    """the arguments with these struct fields set last"""
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def fields(p):
    return tuple(getattr(p, f) for f in T.FIELDS)


@pytest.fixture(scope="module")
def plans():
    """(group, description, plan) of every row of the table, asked once; (a) proves them equal to the pinned ones"""
    return T.collect(L.load())


@pytest.fixture(scope="module")
def table(plans):
    return [dict(zip(T.FIELDS, t)) for t in sorted({t for _, _, t in plans})]


# ---- (a) ------------------------------------------------------------------------------------------------------------------
def test_every_row_of_the_pinned_table(plans):
    pinned = json.load(open(T.TABLE))
    assert pinned["fields"] == list(T.FIELDS) and pinned["codes"] == T.LEGEND and len(plans) > 100000
    bad = T.check(plans, pinned)
    assert not bad, "launches moved (table -> now); if intended, regenerate with tools/igemm_plan_table.py --write:\n" + "\n".join(bad)
    t = list(plans[0][2])
    t[5] += 8                                                # the digest sees a field the letters do not: one grid off by 8
    assert T.check([(plans[0][0], plans[0][1], tuple(t))] + plans[1:], pinned)


def test_the_table_covers_what_it_is_for(table):
    plans = table
    ok = [p for p in plans if p["rc"] == 0]
    assert {p["tile"] for p in ok} == {T128, T192, T256, T320} and {p["kind"] for p in ok} == set(range(9))
    assert {p["rc"] for p in plans} == {0, EINVAL} and all(not any(p[f] for f in T.FIELDS[1:]) for p in plans if p["rc"])
    assert {p["split"] for p in ok} == set(range(1, 9)) and {p["launches"] for p in ok} == {1, 2, 3}
    assert any(p["stats"] and p["split"] > 1 for p in ok) and any(p["stats"] and p["split"] == 1 for p in ok)


# ---- (b) ------------------------------------------------------------------------------------------------------------------
def test_forced_ineligible_tile_is_refused():
    for tile, rc in ((T128, 0), (T192, 0), (T256, EINVAL), (T320, EINVAL)):      # N % 8 != 0: no narrow-store path on 8 waves
        assert plan(T.make_args(1, 12, 64, tile=tile)).rc == rc, tile
    assert plan(T.make_args(1, 12, 64, tile=3)).rc == EINVAL                     # not a MOFA_TILE_*


@pytest.mark.parametrize("s", cc.PIPE_OVER_ROWS, ids=repr)
def test_auto_falls_back_to_192x128_beyond_the_packing_edges(s):
    """the geometry of k3-W1025 / k3-2048img with N = 320 on 8 CUs: one pixel / image less and the model's 8-wave choice runs;
    at the edge the same choice is not eligible and the chain ends on 192x128 (never 128x128); forced, it is refused"""
    def at(W, n):
        return T.make_args(n * s.H * W, 320, 64, 0, L.MODE_CONV3X3, T.conv_geom(s.H, W))
    inside, beyond = (at(s.W - 1, s.n), at(s.W, s.n)) if s.id == "k3-W1025" else (at(s.W, s.n - 1), at(s.W, s.n))
    assert plan(inside, 8).tile in (T256, T320)
    assert fields(plan(beyond, 8))[:2] == (0, T192)
    for tile in (T256, T320):
        beyond.tile = tile
        assert plan(beyond, 8).rc == EINVAL
    assert all(cc.plan(s, epi, n_cu=n).tile in (T128, T192) for epi in cc.EPIS for n in (8, 64, 256, 304))   # the table's own rows


def test_kind_7_never_plans_256x320(table):
    assert not [p for p in table if p["rc"] == 0 and p["kind"] == 7 and p["tile"] == T320]
    assert plan(T.make_args(1, 8, 45 * 64, 3)).tile == T320                     # two residuals: the model's choice (one tile, split) ...
    assert plan(T.make_args(1, 8, 45 * 64, 7)).tile == T128                     # ... plus a row vector: not a candidate of the model
    assert plan(T.make_args(1, 8, 45 * 64, 7, tile=T320)).rc == EINVAL and plan(T.make_args(1, 8, 45 * 64, 7, tile=T256)).rc == 0


def test_geglu_never_splits(table):
    assert not [p for p in table if p["rc"] == 0 and p["kind"] == 8 and (p["split"], p["rem_tiles"], p["launches"]) != (1, 0, 1)]
    plain, geglu = plan(T.make_args(257, 320, 45 * 64, 0, tile=T320)), plan(T.make_args(257, 320, 45 * 64, 8, tile=T320))
    assert (plain.split, plain.rem_tiles, plain.launches) == (5, 2, 2) and (geglu.rc, geglu.split, geglu.launches) == (0, 1, 1)


def test_stats_force_256x320():
    """the a->stats quirk: the tile is forced like a->tile forces it, and a misaligned stats pointer is an error"""
    assert plan(T.make_args(64, 320, 64, 0)).tile == T128
    p = plan(T.make_args(64, 320, 64, 0, stats=True))
    assert (p.rc, p.tile, p.stats, p.launches) == (0, T320, 1, 1)
    p = plan(T.make_args(257 * 64, 320, 45 * 64, 1, stats=True), 304)           # 65 tiles on 304 CUs: split, fix-up, remainder pair sums
    assert (p.rc, p.tile, p.stats, p.split > 1, p.launches) == (0, T320, 1, True, 3)
    for bad in (dict(stats=T.STATS + 8), dict(x=T.X + 8), dict(tile=T256), dict(M=96), dict(N=640 + 8, ldo=648), dict(act=L.ACT_SILU),
                dict(r1=T.R1, ldr1=320, s1=0.5), dict(r2=T.R2, ldr2=320)):
        assert plan(but(T.make_args(64, 320, 64, 0, stats=True), **bad)).rc == EINVAL, bad
    assert L.load().mofa_igemm_stats_ok(ctypes.byref(T.make_args(64, 320, 64, 0))) == 1
    assert L.load().mofa_igemm_stats_ok(ctypes.byref(T.make_args(64, 320, 64, 0, x=T.X + 8))) == 0


def test_unaligned_workspace_is_costed_with_a_split_it_does_not_get():
    """the workspace quirk: the model prices the split for any workspace pointer, the launch declines it for a misaligned one"""
    none, ok, odd = (plan(T.make_args(257, 320, 45 * 64, 0, **kw)) for kw in (dict(ws=False), dict(), dict(workspace=T.WS + 8)))
    assert (none.tile, none.split) == (T128, 1)                                  # without the split the tile does not pay
    assert (ok.tile, ok.split, ok.full_tiles, ok.rem_tiles, ok.grid, ok.launches) == (T320, 5, 0, 2, 16, 2)
    assert (odd.tile, odd.split, odd.full_tiles, odd.rem_tiles, odd.grid, odd.launches) == (T320, 1, 2, 0, 8, 1)


def test_split_work_items_fit_the_grid(table):
    for p in table:
        assert p["rem_tiles"] * p["split"] <= p["grid"] and (p["split"] > 1) == (p["rem_tiles"] > 0), p
        if p["rc"] == 0:
            assert p["full_tiles"] + p["rem_tiles"] == p["tiles_m"] * p["tiles_n"] and p["grid"] % 8 == 0, p


def test_cu_count_is_rounded_down_to_a_multiple_of_8():
    for a in (T.make_args(7200, 1280, 180 * 64, 1), T.make_args(460800, 320, 5 * 64, 0), T.make_args(257, 320, 45 * 64, 0),
              T.make_args(28800, 10240, 20 * 64, 8)):
        assert fields(plan(a, 250)) == fields(plan(a, 248)) and fields(plan(a, 7)) == fields(plan(a, 8)) == fields(plan(a, 1))
    assert fields(plan(T.make_args(460800, 320, 5 * 64, 0), 248)) != fields(plan(T.make_args(460800, 320, 5 * 64, 0), 256))


def test_query_arguments():
    l, a, p = L.load(), T.make_args(256, 320, 64), L.IgemmPlan()
    assert l.mofa_igemm_plan(None, 256, ctypes.byref(p)) == EINVAL and l.mofa_igemm_plan(ctypes.byref(a), 256, None) == EINVAL
    assert l.mofa_igemm_plan(ctypes.byref(a), 0, ctypes.byref(p)) == EINVAL and l.mofa_igemm_plan(ctypes.byref(a), -8, ctypes.byref(p)) == EINVAL
    assert ctypes.sizeof(L.IgemmPlan) == 68 and l.mofa_igemm_plan(ctypes.byref(a), 256, ctypes.byref(p)) == 0 and not any(p.reserved)


# ---- (c) ------------------------------------------------------------------------------------------------------------------
G3 = T.conv_geom(11, 13)
INVALID = [dict(x=None), dict(w=None), dict(out=None), dict(M=0), dict(N=0), dict(Cin=0), dict(Cin=48, ldx=48), dict(N=70), dict(mode=3),
           dict(mode=-1), dict(act=5), dict(act=-1), dict(ldx=68), dict(ldo=74), dict(r1=T.R1, ldr1=74), dict(r2=T.R2, ldr2=74),
           dict(rowvec=T.RV, rv_div=0), dict(rowvec=T.RV, rv_mod_in=0), dict(rowvec=T.RV, rv_mod_out=0),
           dict(act=L.ACT_GEGLU_PAIR), dict(N=128, act=L.ACT_GEGLU_PAIR, r1=T.R1, ldr1=128), dict(N=128, act=L.ACT_GEGLU_PAIR, rowvec=T.RV),
           dict(tile=1), dict(tile=7), dict(stats=T.STATS),
           dict(mode=L.MODE_CONV3X3), dict(geom=G3, Hin=0), dict(geom=G3, Wout=0), dict(geom=G3, stride=3), dict(geom=G3, up=0),
           dict(geom=G3, ksize=2), dict(geom=G3, ksize=9), dict(geom=G3, dil=-1), dict(geom=G3, dil=2, up=2), dict(geom=G3, pad=2),
           dict(geom=G3, M=144), dict(geom=T.conv_geom(65536, 1), M=65536), dict(geom=T.conv_geom(1, 65536), M=65536),
           dict(mode=L.MODE_CONVT3, T=-1, HW=11), dict(mode=L.MODE_CONVT3, T=2, HW=0), dict(mode=L.MODE_CONVT3, T=4, HW=11)]


def test_plan_validation_is_the_launchers():
    """one violated rule at a time on otherwise valid, never dereferenced addresses (the empty struct of test_abi_cpu.py and the
    Cin % 64 != 0 of test_kernels_gpu.py::test_igemm_rejects_bad_args among them): mofa_igemm_f16 returns MOFA_EINVAL before it
    looks for a device, and the plan carries the same code.  The valid call is not launched here: it is MOFA_ELAUNCH without a
    device, so only its plan is asked"""
    l = L.load()
    assert plan(L.IgemmArgs()).rc == l.mofa_igemm_f16(ctypes.byref(L.IgemmArgs()), None) == EINVAL
    assert plan(T.make_args(143, 72, 64, mode=L.MODE_CONV3X3, geom=G3)).rc == 0
    for bad in INVALID:
        kw = dict(bad)
        geom = kw.pop("geom", None)
        a = but(T.make_args(143, 72, 64, mode=L.MODE_CONV3X3 if geom else L.MODE_PLAIN, geom=geom), **kw)
        assert plan(a).rc == l.mofa_igemm_f16(ctypes.byref(a), None) == EINVAL, bad


# ---- (d) ------------------------------------------------------------------------------------------------------------------
def test_planner_is_host_code():
    hdr = os.path.join(ROOT, "mofa_video_amd", "csrc", "igemm_plan.h")
    includes = [ln.split()[1] for ln in open(hdr) if ln.startswith("#include")]
    assert includes == ["<stdint.h>", '"../../include/mofa_hip.h"'], includes
    r = subprocess.run([shutil.which("g++") or "g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-include", hdr, os.devnull],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
