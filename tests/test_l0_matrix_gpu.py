"""The case table of tests/l0_cases.py through ``mofa_video_amd.ops`` on the GPU: the two hand-scheduled level-0 kernels,
``lin320`` (csrc/lin320.hip) and ``ff320`` (csrc/ff320.hip), on exact sums, row edges, ring phases and poisoned rows.

  a  lin320, exact-grid data and exact LayerNorm rows: the output is bit-equal to round16(round16(s_acc * acc) + s1 * r1)
     computed in fp64 (l0_cases docstring: why no summation order can change a bit), on all eight template instances, N of 1 to
     15 chunks (the look-ahead wrap with 2, 3, 4 and 6 chunks), M at 1, 8 k +- 1, the wave, the tile and inside the last wave of
     a second tile
  b  lin320, a block of 333 rows repeated until some workgroup processes FOUR tiles (the grid is the device's compute-unit
     count, as the launcher sizes it): the ring counter g does not restart at a tile boundary, so the tiles of a workgroup
     start at ring phases 0, 2, 1, 0 (N = 320, 128) / 0, 1, 2, 0 (N = 64) -- rows [0, 333) against the fp64 reference, and every
     later repeat bit-equal to the first (one torch.equal): a row's value depends on that row alone, and its summation order
     is fixed per lane pair and MFMA column, whatever tile, wave or ring slot it lands in
  c  ff320 likewise with three tiles per workgroup (steps 40 / 41 of a tile prefetch the next tile's W1(0) / W1(1); the b1
     hand-over at the tile boundary crossed twice)
  d  ff320 at M = 1, 31, 32, 33, 127, 128, 129, 225 on five instances, all buffers guarded
  e  row isolation: row 0 all NaN (the row every out-of-range lane reads instead of its own), row M - 1 all NaN, one +inf at a
     wave boundary -- every other row, and every guard word, bit-equal to the clean run

Every case: guards intact (NaN rows and columns around every view, compared as bits), read-only arguments bit-unchanged, the
returned tensors ARE the ``out`` / ``ln_out`` buffers.  Exact cases compare bits, the others take the project's stated
tolerances from ``op_cases.TOL``.  A failure names the first offending (row, column) and its tile, wave, row group, chunk and
ring slot.  tests/test_l0_cases_cpu.py proves on the CPU that each check fails on a wrong kernel.  ``test_worst_ratio`` prints
one ``L0-WORST <op>/<matrix>: err / bound`` line per matrix (pytest -s)."""
import collections

import pytest
import torch

import l0_cases as lc
import op_cases as oc

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = collections.defaultdict(float)
STATIC = [c for c in lc.CASES if c.matrix in "ad"]
ISO = [c for c in lc.CASES if c.matrix == "e"]


@pytest.fixture(scope="module")
def ops():
    from mofa_video_amd import lib
    from mofa_video_amd import ops as o
    lib.load()
    return o


@pytest.fixture(scope="module")
def cus():
    """what csrc/common.h's LaunchSetup sizes the persistent grids from"""
    return torch.cuda.get_device_properties(0).multi_processor_count


def _check(ops, case, cus=None):
    r = oc.run(ops, case, DEV)
    worst, errs = lc.check_run(case, r, cus)
    key = f"{case.op}/{case.matrix}"
    WORST[key] = max(WORST[key], worst)
    print(f"L0 {case.id}: " + ("bit-equal" if case.tol == "exact" and not errs else f"worst err / bound {worst:.3f}"))
    assert not errs, errs
    return r


@pytest.mark.parametrize("case", STATIC, ids=repr)
def test_exact_sums_and_row_edges(ops, case):
    _check(ops, case)


@pytest.mark.parametrize("inst,N,data", lc.PERIODIC_LIN, ids=lambda v: "".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_lin320_ring_phases_by_periodic_rows(ops, cus, inst, N, data):
    case = lc.periodic_lin(inst, N, data, cus, DEV)
    ntiles = -(-case.meta["M"] // 256)
    assert ntiles >= (2 if N == 960 else 3) * cus + 1
    _check(ops, case, cus)


@pytest.mark.parametrize("kind", lc.PERIODIC_FF)
def test_ff320_ring_phases_by_periodic_rows(ops, cus, kind):
    case = lc.periodic_ff(kind, cus, DEV)
    assert -(-case.meta["M"] // 128) >= 2 * cus + 1
    _check(ops, case, cus)


@pytest.mark.parametrize("clean", [c for c in ISO if c.meta["poison"] is None], ids=repr)
def test_row_isolation(ops, clean):
    base = _check(ops, clean)
    stem = clean.id.rsplit("-M", 1)[0]
    poisoned = [c for c in ISO if c.meta["poison"] and c.id.rsplit("-M", 1)[0] == stem]
    assert len(poisoned) == 3
    for c in poisoned:
        r = _check(ops, c)
        errs = lc.isolation_errors(c, r, base)
        assert not errs, errs


def test_worst_ratio():
    for key in sorted(WORST):
        print(f"L0-WORST {key}: {WORST[key]:.3f}")
