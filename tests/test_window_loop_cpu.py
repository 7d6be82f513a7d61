"""The bookkeeping of the Keypoint window loop without a network: ``pipeline.WindowPlan`` (overlap average, the frontier of final
frames, the decode chunks below it) against brute force and against the reference's formula
(MOFA-Video-Keypoint/pipeline/svdxt_pipeline_ctrlnet_loop.py:502-511: ``value[...] += window`` in view order, ``/ count``), and
``pipeline.window_layout`` against the tuples the loop derived inline before the planner existed.

Two "wrong planner" mutants show that the checks can fail (as tests/test_aux_cases_cpu.py does for the kernels):
  early-final   a frame is final one view before its last covering view is merged      fails the frontier check
  reverse-sum   the views are summed last to first                                     fails the bit-equality check wherever a
                                                                                       frame has three or more covering views
"""
import pytest
import torch

from mofa_video_amd.parallel import FrameParallel, GroupedWindowParallel, Layout, ThreadComm, ThreadWorld, WindowParallel
from mofa_video_amd.pipeline import WindowPlan, window_layout, window_views

CASES = [(4, 4, 2, 2),        # one window = the clip: the views (1,4), (1,4)
         (6, 4, 2, 2), (8, 4, 2, 2), (10, 4, 2, 2),
         (7, 4, 3, 2),        # the last view repeats
         (9, 4, 3, 4),        # an irregular last view, a partial last chunk
         (49, 25, 12, 8), (97, 25, 12, 8)]


def _covers(idx, view, f):
    """view ``idx`` writes frame f: the first view brings frame 0 along"""
    return (0 if idx == 0 else view[0]) <= f < view[1]


class EarlyFinal(WindowPlan):
    def frontier(self, m):
        return super().frontier(min(m + 1, len(self.views)))


class ReverseSum(WindowPlan):
    def accumulations(self, m, since=0):
        seen, out = set(), []
        for idx, src, f, _ in reversed(super().accumulations(m, since)):
            out.append((idx, src, f, f not in seen))
            seen.add(f)
        return out


def check_tables(plan, views, N, chunk):
    assert plan.count == [sum(_covers(i, v, f) for i, v in enumerate(views)) for f in range(N)]
    for m in range(len(views) + 1):
        later = [f for f in range(N) for i, v in enumerate(views) if i >= m and _covers(i, v, f)]
        F = min(later) if later else N                     # the largest F with no unmerged view on a frame below F
        assert plan.frontier(m) == F, (m, plan.frontier(m), F)
        assert plan.ready_chunks(m) == [ci for ci in range(-(-N // chunk)) if min(ci * chunk + chunk, N) - 1 < F], m


def check_average(plan, views, N):
    """the accumulation list applied with plain torch arithmetic == the reference's formula, bit for bit"""
    g = torch.Generator().manual_seed(N)
    wins = [torch.randn(v[1] - v[0] + 1, 5, generator=g) for v in views]          # frame 0 + the frames [t0, t1) of every view
    ref = torch.zeros(N, 5)
    for i, (t0, t1) in enumerate(views):                   # :502-507
        if i == 0:
            ref[0:t1] += wins[i]
        else:
            ref[t0:t1] += wins[i][1:]
    ref = ref / torch.tensor(plan.count, dtype=torch.float32)[:, None]            # :511
    value = torch.full((N, 5), float("nan"))
    for idx, src, f, first in plan.accumulations(len(views)):
        value[f] = wins[idx][src] if first else value[f] + wins[idx][src]
    got = value / torch.tensor(plan.count, dtype=torch.float32)[:, None]
    assert torch.equal(got, ref)


@pytest.mark.parametrize("N,window,stride,chunk", CASES)
def test_plan_against_brute_force(N, window, stride, chunk):
    views = window_views(N, window, stride)
    assert views[0][0] == 1 and views[-1][1] == N
    plan = WindowPlan(views, N, chunk)
    check_tables(plan, views, N, chunk)
    check_average(plan, views, N)
    # merged piecewise, as the last step does when its rounds finish one after the other: the same list
    cuts = list(range(len(views) + 1))
    assert sum((plan.accumulations(b, since=a) for a, b in zip(cuts, cuts[1:])), []) == plan.accumulations(len(views))
    assert plan.frontier(0) == 0 and plan.frontier(len(views)) == N and min(plan.count) >= 1


def test_case_table_holds_its_edges():
    v = {c: window_views(c[0], c[1], c[2]) for c in CASES}
    assert v[(4, 4, 2, 2)] == [(1, 4), (1, 4)]
    assert v[(7, 4, 3, 2)][-1] == v[(7, 4, 3, 2)][-2]                               # a repeated last view
    assert v[(9, 4, 3, 4)][-1] == (6, 9) and 9 % 4 != 0                            # irregular last view, partial last chunk
    assert max(WindowPlan(v[(97, 25, 12, 8)], 97, 8).count) >= 3                    # (what the reverse-sum mutant needs)
    with pytest.raises(ValueError, match="first window"):
        WindowPlan([(2, 5)], 5, 2)


def test_mutants_fail():
    caught = {"early-final": 0, "reverse-sum": 0}
    for N, window, stride, chunk in CASES:
        views = window_views(N, window, stride)
        with pytest.raises(AssertionError):                # every case: view 0's frames are final only once view 0 is merged
            check_tables(EarlyFinal(views, N, chunk), views, N, chunk)
        caught["early-final"] += 1
        check_average(WindowPlan(views, N, chunk), views, N)
        try:
            check_average(ReverseSum(views, N, chunk), views, N)
            assert max(WindowPlan(views, N, chunk).count) <= 2, (N, window, stride)   # a + b == b + a: no defect to see there
        except AssertionError:
            assert max(WindowPlan(views, N, chunk).count) >= 3, (N, window, stride)
            caught["reverse-sum"] += 1
    print(f"WINDOW-MUTANT caught: {caught}")
    assert caught["early-final"] == len(CASES) and caught["reverse-sum"] >= 3


def test_window_layout():
    """(framepar, wpar, world, rank, nslots, slot) for every ``parallel`` the window loop takes"""
    assert tuple(window_layout(None, 4)) == (None, None, 1, 0, 1, 0)
    wp = WindowParallel(ThreadComm(ThreadWorld(3), 1), 1, 3)
    assert tuple(window_layout(wp, 4)) == (None, wp, 3, 1, 3, 1)
    for r in range(4):
        fp = FrameParallel(Layout(4, r, 4), ThreadComm(ThreadWorld(4), r))
        assert tuple(window_layout(fp, 4)) == (fp, None, 4, r, 1, 0)
    with pytest.raises(ValueError, match="Layout was built for 4 frames"):
        window_layout(FrameParallel(Layout(4, 0, 4), ThreadComm(ThreadWorld(4), 0)), 5)
    gp = GroupedWindowParallel(ThreadComm(ThreadWorld(8), 5), 5, 8, 4, 4)
    assert tuple(window_layout(gp, 4)) == (gp.frame, gp, 8, 5, 2, 1)
    assert (gp.frame.lay.rank, gp.frame.lay.base, gp.frame.lay.world) == (1, 4, 4)
