"""mofa_attn_temporal_long_f16 (csrc/attention.hip attn_temporal_long_kernel): temporal attention over 33 ... 128 frames, driven
through ``ops.attn_temporal`` so that the dispatch is what is tested (tests/attn_long_cases.py: the families, the guards and the
checks; tests/test_temporal_long_cpu.py runs the same cases through the CPU stand-in).

T around every 32-key tile edge (33, 63 / 64 / 65, 95 / 96 / 97, 125, 127 / 128) x head_dim 64 / 128 x three geometries whose
sequence counts (1, 20, 14) leave the last workgroup partly empty for 2 and 4 waves per workgroup.  Every argument is a guarded
view with its own leading dimension; the guards must be intact afterwards."""
import pytest
import torch

import attn_cases as ac
import attn_long_cases as lc
from op_cases import same_bits

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
    lc.release()


def _family(ops, form, hd, T, geoms=lc.LONG_GEOM):
    top, bad = 0.0, []
    for HW, heads, clips in geoms:
        case = lc.long_case(form, T, hd, HW, heads, clips)
        worst, errs = lc.check_long(case, lc.run(ops, case, DEV))
        top, bad = max(top, worst), bad + errs
    return top, bad


@pytest.mark.parametrize("T", lc.LONG_T)
@pytest.mark.parametrize("hd", lc.LONG_HD)
def test_random_operands_against_fp64(ops, hd, T):
    top, bad = _family(ops, "gauss", hd, T)
    print(f"ATTN-LONG gauss hd{hd} T{T}: worst err / bound {top:.3f}")
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("T", lc.LONG_T)
@pytest.mark.parametrize("hd", lc.LONG_HD)
def test_exact_selection(ops, hd, T):
    """out[i] == v[pi(i)] element for element: every query block reaches into every key tile"""
    lc.assert_selection_perm(T)
    top, bad = _family(ops, "select", hd, T)
    print(f"ATTN-LONG select hd{hd} T{T}: " + ("equal by value" if not bad else "DIFFERS"))
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("T", lc.LONG_T)
@pytest.mark.parametrize("hd", lc.LONG_HD)
def test_key_count(ops, hd, T):
    """uniform probabilities: 1 / T to one fp16 ulp from a single 1.0 in frame T-1, and a constant value returned exactly"""
    top, bad = _family(ops, "count-one", hd, T)
    print(f"ATTN-LONG count-one hd{hd} T{T}: worst distance from 1 / T {top:.3f} fp16 ulp")
    _, bad_c = _family(ops, "count-c", hd, T)
    assert not bad + bad_c, (len(bad + bad_c), (bad + bad_c)[:8])


@pytest.mark.parametrize("T", lc.LONG_T)
@pytest.mark.parametrize("hd", lc.LONG_HD)
def test_phantom_keys(ops, hd, T):
    """clip 0's output is the same bit for bit whether the rows that follow it -- clip 1's K / V -- hold ordinary values or
    winning keys with NaN values; for the last clip the NaN guard rows of every other test play that role"""
    for HW, heads, clips in [g for g in lc.LONG_GEOM if g[2] == 2]:
        outs = []
        for form in ("phantom-plain", "phantom-decoy"):
            case = lc.long_case(form, T, hd, HW, heads, clips)
            r = lc.run(ops, case, DEV)
            worst, errs = lc.check_long(case, r)
            assert not errs, errs
            outs.append(r.placed["out"].t[:T * HW].clone())
        assert same_bits(outs[0], outs[1]), f"hd{hd} T{T} HW{HW}: clip 0 depends on clip 1's keys"


@pytest.mark.parametrize("T", (1, 25, 32))
@pytest.mark.parametrize("hd", lc.LONG_HD)
def test_agrees_with_the_shipped_kernel_where_both_apply(ops, hd, T):
    """the new entry point called directly at T <= 32 (ops.attn_temporal sends those lengths to the shipped kernel): both within
    the tolerance of fp64"""
    from mofa_video_amd import lib as L
    HW, heads, clips = 5, 2, 2
    case = lc.long_case("gauss", T, hd, HW, heads, clips)
    d = case.data()
    r = lc.run(ops, case, DEV)                                      # the shipped kernel
    worst_s, errs = lc.check_long(case, r)
    assert not errs, errs
    kw = r.kwargs
    out = torch.full_like(r.placed["out"].buf, float("nan"))
    view = r.placed["out"].cut(out)
    L.check(L.load().mofa_attn_temporal_long_f16(kw["q"].data_ptr(), kw["k"].data_ptr(), kw["v"].data_ptr(), view.data_ptr(), clips, T, HW,
                                                 heads, hd, kw["q"].stride(0), kw["k"].stride(0), view.stride(0), hd ** -0.5,
                                                 L.stream_ptr()), "mofa_attn_temporal_long_f16")
    torch.cuda.synchronize()
    worst_l, msg = lc.close_errors(view.cpu(), d.expect, lc.TOL["attn_temporal"], case.id + " (long entry point)")
    diff = (view.float() - r.placed["out"].t.float()).abs().max().item()
    print(f"ATTN-LONG hd{hd} T{T}: worst err / bound shipped {worst_s:.3f}, long {worst_l:.3f}; max |long - shipped| {diff:.3e}")
    assert msg is None, msg
    inside = r.placed["out"].inside
    assert bool(torch.isnan(out[~inside]).all()), "the long entry point wrote outside its out view"


def _randn16(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV).half()


@pytest.mark.parametrize("hd,T,HW,heads,clips", [(64, 48, 2304, 5, 2), (128, 96, 576, 10, 2)])
def test_repeat_launches_bit_identical(ops, hd, T, HW, heads, clips):
    """a chip-filling launch: a key tile read before the wave's LDS writes landed, or a wave reaching into its neighbour's LDS
    region, shows as a run-to-run difference"""
    Cc, rows = heads * hd, clips * T * HW
    q, k, v = (_randn16(rows, Cc, seed=s) for s in (1, 2, 3))
    first = ops.attn_temporal(q, k, v, clips, T, HW, heads, head_dim=hd)
    split = lambda t: t.reshape(clips, T, HW, heads, hd).permute(0, 2, 3, 1, 4)
    ref = ac.attention64(split(q), split(k), split(v), hd ** -0.5, device=DEV, chunk=2048, keep=True)
    ref = ref.permute(0, 3, 1, 2, 4).reshape(rows, Cc)
    worst, msg = lc.close_errors(first, ref, lc.TOL["attn_temporal"], f"hd{hd} T{T} HW{HW}")
    print(f"ATTN-LONG repeat hd{hd} T{T} HW{HW}: worst err / bound {worst:.3f}")
    assert msg is None, msg
    for i in range(6):
        again = ops.attn_temporal(q, k, v, clips, T, HW, heads, head_dim=hd)
        assert torch.equal(again, first), f"launch {i + 2} differs from the first"


def test_rejections_through_lib_check(ops):
    from mofa_video_amd import lib as L
    from mofa_video_amd.lib import MofaHipError
    l = L.load()
    t = torch.zeros(129 * 2, 160 + 16, dtype=torch.float16, device=DEV)

    def call(T=33, hd=64, ld=176, ldkv=176, ldo=176):
        L.check(l.mofa_attn_temporal_long_f16(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), 1, T, 1, 1, hd, ld, ldkv, ldo,
                                              0.125, L.stream_ptr()), "mofa_attn_temporal_long_f16")
    for bad in (dict(T=129), dict(hd=80), dict(ldo=12)):
        with pytest.raises(MofaHipError, match=r"mofa_attn_temporal_long_f16 failed with code -22$"):
            call(**bad)
    q = _randn16(33 * 3, 64, seed=5)
    out = ops.attn_temporal(q, q, q, 1, 33, 3, 1)                    # no longer refused
    torch.cuda.synchronize()
    assert out.shape == (99, 64) and bool(torch.isfinite(out).all())
    with pytest.raises(ValueError, match="frame-sharded clips are limited to 32 key slots"):
        ops.attn_temporal(q, q, q, 1, 33, 3, 1, key_mask=1)
