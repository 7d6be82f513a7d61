"""The attention kernels of csrc/attention.hip at the sequence lengths where their structure changes, against fp64 and -- for the
one-hot family -- by EQUALITY (tests/attn_cases.py: the tables, the three input families, the guards and the checks;
tests/test_attn_cases_cpu.py proves the same cases and the checks' ability to fail on the CPU).

Spatial: the three instantiations <64,1>, <64,2>, <128,1> at S around the 64-key tile, the 32-row wave block and the 128- /
256-row workgroup, with work counts below 8, equal to 8, multiples of 8 and -- over the three together -- every remainder of the
deal over the 8 XCDs; and the launcher's own choice at S = 240 / 241, either side of its rule, where <64,2> meets a half-empty
query block and a ragged last key tile.  Temporal: T around the 16-key MFMA step and the 32-row tile, partial last workgroups,
Tq < T, four mask shapes with the masked frames' rows holding NaN or finite decoys.  Repeat launches at chip-filling shapes must
be bit-identical.  (That the tables hold these classes is asserted once, in tests/test_attn_cases_cpu.py.)"""
import pytest
import torch

import attn_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from mofa_video_amd import lib
    from mofa_video_amd import ops as o
    lib.load()
    return o


@pytest.fixture(scope="module", autouse=True)
def _release_case_data():
    yield
    ac.release()


def _check(ops, case):
    worst, errs = ac.check_run(case, ac.run(ops, case, DEV))
    print(f"ATTN-EDGE {case.id}: " + ("equal by value" if case.tol == "exact" and not errs else f"worst err / bound {worst:.3f}"))
    return worst, errs


@pytest.mark.parametrize("form", ac.SPATIAL_FORMS)
@pytest.mark.parametrize("S,heads,frames", ac.spatial_shapes())
@pytest.mark.parametrize("hd,qb", ac.SPATIAL_INST)
def test_spatial_matrix(ops, hd, qb, S, heads, frames, form):
    _, errs = _check(ops, ac.spatial_case(hd, qb, S, heads, frames, form))
    assert not errs, errs


@pytest.mark.parametrize("form", ac.AUTO_FORMS)
@pytest.mark.parametrize("S", ac.AUTO_S)
def test_spatial_auto_dispatch(ops, S, form):
    """query_blocks=0 at 1024 frames of one head: the launcher's rule takes 128-row workgroups at S = 240 and 256-row ones at
    S = 241 (its first ragged length) -- the production-reachable <64,2> with query rows 241 ... 255 beyond S and 49 real keys
    in the last tile.  Which kernel ran is not looked at: both lengths owe the same checks"""
    _, errs = _check(ops, ac.spatial_case(64, 0, S, ac.AUTO_HEADS, ac.AUTO_FRAMES, form, big=True, device=DEV))
    assert not errs, errs


@pytest.mark.parametrize("T", ac.TEMPORAL_T)
@pytest.mark.parametrize("hd", ac.TEMPORAL_HD)
def test_temporal_matrix(ops, hd, T):
    """every (Tq, mask, fill, family) of one (head_dim, T); the worst ratio per tolerance class is printed"""
    cases = ac.temporal_cases(hd, T)
    top, bad = {}, []
    for case in cases:
        worst, errs = ac.check_run(case, ac.run(ops, case, DEV))
        top[case.tol] = max(top.get(case.tol, 0.0), worst)
        bad += errs
    print(f"ATTN-EDGE temporal hd{hd} T{T}: {len(cases)} cases, worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in top.items()))
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("hd", ac.TEMPORAL_HD)
def test_temporal_rejects_empty_mask_and_long_queries(ops, hd):
    """the launcher's own MOFA_EINVAL (-22) through lib.check, not just any error: a call that is valid but for the one argument"""
    from mofa_video_amd.lib import MofaHipError
    T = 16
    kw = ac.run(ops, ac.temporal_case(hd, T, T, "A"), DEV).kwargs
    ops.attn_temporal(**dict(kw, key_mask=1))                       # the same call is accepted with one key left
    einval = dict(expected_exception=MofaHipError, match=r"mofa_attn_temporal(_masked)?_f16 failed with code -22$")
    with pytest.raises(**einval):
        ops.attn_temporal(**dict(kw, key_mask=0))
    with pytest.raises(**einval):                                   # bits >= T only: nothing is left once the launcher clears them
        ops.attn_temporal(**dict(kw, key_mask=0xffff0000))
    with pytest.raises(**einval):                                   # (the buffers hold T query frames; the call must not start)
        ops.attn_temporal(**dict(kw, T=T - 1, Tq=T))


# ---- repeat launches: six more launches bit-identical to the first, the first within tolerance of fp64 ----------------------
def _randn16(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV).half()


def _assert_close(out, ref, tol, what):
    worst, msg = ac.close_errors(out, ref, tol, what)
    print(f"ATTN-EDGE {what}: worst err / bound {worst:.3f}")
    assert msg is None, msg


@pytest.mark.parametrize("hd,qb,S,heads,frames", [(64, 1, 2304, 5, 10), (64, 2, 2304, 5, 10), (128, 1, 576, 10, 10)])
def test_spatial_repeat_launches_bit_identical(ops, hd, qb, S, heads, frames):
    """the double-buffered K / V tiles (LDS-DMA with one vmcnt(0) before the barrier for head_dim 64) at a shape that fills the
    chip: a tile read before it landed, or overwritten while still read, shows as a run-to-run difference"""
    Cc = heads * hd
    q, k, v = (_randn16(frames * S, Cc, seed=200 + i) for i in range(3))
    first = ops.attn_spatial(q, k, v, frames, heads, S, head_dim=hd, query_blocks=qb).clone()
    for i in range(6):
        again = ops.attn_spatial(q, k, v, frames, heads, S, head_dim=hd, query_blocks=qb)
        assert torch.equal(again, first), f"launch {i + 2} differs from the first in {int((again != first).sum())} elements"
    Q, K, V = (t.reshape(frames, S, heads, hd).permute(0, 2, 1, 3) for t in (q, k, v))
    ref = ac.attention64(Q, K, V, hd ** -0.5, device=DEV, chunk=5, keep=True).permute(0, 2, 1, 3).reshape(frames * S, Cc)
    _assert_close(first, ref, ac.TOL["attn_spatial"], f"repeat spatial hd{hd} qb{qb}")


def test_temporal_repeat_launches_bit_identical(ops):
    T, HW, heads, clips, hd = 25, 2304, 5, 2, 64
    Cc = heads * hd
    q, k, v = (_randn16(clips * T * HW, Cc, seed=210 + i) for i in range(3))
    first = ops.attn_temporal(q, k, v, clips, T, HW, heads, head_dim=hd).clone()
    for i in range(6):
        again = ops.attn_temporal(q, k, v, clips, T, HW, heads, head_dim=hd)
        assert torch.equal(again, first), f"launch {i + 2} differs from the first in {int((again != first).sum())} elements"
    Q, K, V = (t.reshape(clips, T, HW, heads, hd).permute(0, 2, 3, 1, 4) for t in (q, k, v))
    ref = ac.attention64(Q, K, V, hd ** -0.5, device=DEV, chunk=4096, keep=True).permute(0, 3, 1, 2, 4).reshape(clips * T * HW, Cc)
    _assert_close(first, ref, ac.TOL["attn_temporal"], "repeat temporal")
