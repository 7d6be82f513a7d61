"""The attention edge tables of tests/attn_cases.py proven on the CPU before a GPU sees them: the tables hold the classes they are
there for, every precondition of the exact and the sink family holds, every case passes its checks through the torch stand-ins
of tests/emu_ops.py (family C by EQUALITY), and every "wrong attention" mutant FAILS them -- a checker that cannot fail proves
nothing.  tests/test_attn_edges_gpu.py runs the same cases through the HIP kernels."""
import pytest
import torch

import attn_cases as ac
import emu_ops


@pytest.fixture(scope="module", autouse=True)
def _release_case_data():
    yield
    ac.release()


def _checked(module, case):
    r = ac.run(module, case, "cpu")
    worst, errs = ac.check_run(case, r)
    return worst, errs, r.placed["out"].t


def test_tables_hold_their_classes():
    ac.assert_spatial_table()
    ac.assert_temporal_table()


# ---- every case through the stand-ins, with its preconditions --------------------------------------------------------------
def _assert_preconditions(case):
    st = case.data().stats
    if case.form == "B":
        lo, hi = ac.B_LOGIT_RANGE_WIDE if case.big else ac.B_LOGIT_RANGE          # the wide one for the auto-dispatch pair alone
        assert st["range"] == (lo, hi) and lo <= st["lo"] and st["hi"] <= hi, (case.id, st)
    if case.form.startswith("C"):
        assert st["others"] < ac.C_OTHERS_MAX and st["match"] <= ac.C_MATCH_LOGIT_MAX, (case.id, st)
    return st


@pytest.mark.parametrize("S,heads,frames", ac.spatial_shapes())
@pytest.mark.parametrize("hd,qb", ac.SPATIAL_INST)
def test_spatial_stand_in(hd, qb, S, heads, frames):
    for form in ac.SPATIAL_FORMS:
        case = ac.spatial_case(hd, qb, S, heads, frames, form)
        st = _assert_preconditions(case)
        worst, errs, _ = _checked(emu_ops, case)
        print(f"ATTN-CPU {case.id}: worst err / bound {worst:.3f}; logits [{st['lo']:.2f}, {st['hi']:.2f}]"
              + (f", others / match {st['others']:.1e}, gap {st['gap']:.1f} nats" if form.startswith("C") else ""))
        assert not errs, errs


@pytest.mark.parametrize("form", ac.AUTO_FORMS)
@pytest.mark.parametrize("S", ac.AUTO_S)
def test_spatial_auto_dispatch_stand_in(S, form):
    case = ac.spatial_case(64, 0, S, ac.AUTO_HEADS, ac.AUTO_FRAMES, form, big=True)
    _assert_preconditions(case)
    worst, errs, _ = _checked(emu_ops, case)
    print(f"ATTN-CPU {case.id}: worst err / bound {worst:.3f}")
    assert not errs, errs


@pytest.mark.parametrize("T", ac.TEMPORAL_T)
@pytest.mark.parametrize("hd", ac.TEMPORAL_HD)
def test_temporal_stand_in(hd, T):
    cases = ac.temporal_cases(hd, T)
    assert {c.mask for c in cases} == set(ac.temporal_masks(T)) and len({c.id for c in cases}) == len(cases)
    top, bad = 0.0, []
    for case in cases:
        _assert_preconditions(case)
        worst, errs, _ = _checked(emu_ops, case)
        top, bad = max(top, worst), bad + errs
    print(f"ATTN-CPU temporal hd{hd} T{T}: {len(cases)} cases, worst err / bound {top:.3f}")
    assert not bad, bad[:5]


# ---- mutants ---------------------------------------------------------------------------------------------------------------
def _mutant_verdicts(cases, truth_mod, wrong_mod):
    """{form: (worst, errs, equal to the truth's output)}"""
    res = {}
    for form, case in cases.items():
        _, terrs, tout = _checked(truth_mod, case)
        assert not terrs, ("the plain fp64 attention must pass", terrs)
        worst, errs, out = _checked(wrong_mod, case)
        res[form] = (worst, errs, ac.oc.same_bits(out, tout))
    return res


def _assert_mutant(defect, differs, res, what):
    if not differs:                       # the defect is no defect at this length: asserted equal, not skipped
        assert all(same and not errs for _, errs, same in res.values()), (what, defect)
        return
    assert any(errs for _, errs, _ in res.values()), f"{what}: mutant {defect} passes families A + B + C"
    if defect == "swap-v":
        assert all(res[f][1] for f in res if f.startswith("C")), f"{what}: mutant {defect} passes family C"
    if defect in ("phantom", "mask-late"):
        assert res["B"][0] >= 10.0, f"{what}: mutant {defect} fails family B by {res['B'][0]:.1f} x the bound only"


@pytest.mark.parametrize("S,heads,frames", ac.spatial_shapes())
@pytest.mark.parametrize("hd", (64, 128))
def test_spatial_mutants_fail(hd, S, heads, frames):
    cases = {form: ac.spatial_case(hd, 1, S, heads, frames, form) for form in ac.SPATIAL_FORMS}
    for defect in ac.SPATIAL_MUTANTS:
        if defect == "drop-last" and S == 1:
            continue                      # attention over no key at all is undefined
        res = _mutant_verdicts(cases, ac.wrong_spatial(None), ac.wrong_spatial(defect))
        _assert_mutant(defect, ac.mutant_differs(defect, S, 64), res, f"hd{hd} S{S}")
        print(f"ATTN-MUTANT spatial hd{hd} S{S} {defect}: " + ", ".join(f"{f} {w:.1f}" for f, (w, _, _) in res.items()))


@pytest.mark.parametrize("T", ac.TEMPORAL_T)
@pytest.mark.parametrize("hd", ac.TEMPORAL_HD)
def test_temporal_mutants_fail(hd, T):
    cases = {form: ac.temporal_case(hd, T, T, form) for form in ac.TEMPORAL_FORMS}
    for defect in ac.SPATIAL_MUTANTS:
        if defect == "drop-last" and T == 1:
            continue
        res = _mutant_verdicts(cases, ac.wrong_temporal(None), ac.wrong_temporal(defect))
        _assert_mutant(defect, ac.mutant_differs(defect, T, 32), res, f"hd{hd} T{T}")
    # the mask read one bit off: under every mask shape and both fills of the masked rows
    for mask in ("full", "no0", "one", "alt"):
        if mask not in ac.temporal_masks(T):
            continue
        if ac.shifted_mask(ac.temporal_masks(T)[mask][0], T) == 0:
            assert T <= 2                 # no key left: undefined, as the last key dropped at S = 1
            continue
        for fill in (ac.FILLS if mask != "full" else ac.FILLS[:1]):
            cases = {form: ac.temporal_case(hd, T, T, form, mask, fill) for form in ac.TEMPORAL_FORMS}
            res = _mutant_verdicts(cases, ac.wrong_temporal(None), ac.wrong_temporal("mask-shift"))
            assert any(errs for _, errs, _ in res.values()), f"hd{hd} T{T} {mask} {fill}: mutant mask-shift passes A + B + C"
            if fill == "decoy" or mask == "full":   # finite wrong numbers: the exact family names them
                assert all(res[f][1] for f in res if f.startswith("C")), f"hd{hd} T{T} {mask} {fill}: mask-shift passes family C"


def test_truth_is_not_a_mutant():
    """the fp64 attention the mutants are made from agrees with the stand-in inside the stand-in's own fp16 rounding"""
    case = ac.spatial_case(64, 1, 300, 3, 7, "A")
    _, _, a = _checked(ac.wrong_spatial(None), case)
    _, _, b = _checked(emu_ops, case)
    assert (a.float() - b.float()).abs().max().item() <= 2.0 ** -10 * a.float().abs().max().item()
