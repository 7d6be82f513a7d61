"""The case table of tests/l0_cases.py proven on the CPU before a GPU sees it: the table holds the shapes and instances it is
there for, the exact families are exact, the stand-ins of tests/emu_ops.py pass every case -- and every "wrong kernel" mutant
FAILS the check on exactly the cases where the geometry says it must (a checker that cannot fail proves nothing).
tests/test_l0_matrix_gpu.py runs the same cases through the HIP kernels.  Matrices b and c run here on a grid of
``l0_cases.CPU_CUS`` = 2 workgroups, a few periods long: the same tile -> workgroup -> ring phase arithmetic at a smaller M.

The mutants (l0_cases.MUTANTS; l0_cases.mutant_effect states from the geometry alone what each does on a case):
  drop-kstep              lin320: k-step 7 of chunk 1 left out                      every lin320 case
  stale-chunk-third-tile  chunk 1 computed on chunk 0's weights, in the third       matrices b and c only (N > 64), where a
                          tile of a workgroup only                                  workgroup has a third tile
  bias-wrong-chunk        lin320: chunk c takes the bias piece of chunk c + 1       a bias and more than one chunk
  single-rounding         lin320: f16(s_acc * acc + s1 * r1)                        caught on exact data with a residual; WITHIN the
                                                                                    tolerance on Gaussian data (asserted: that is
                                                                                    why the exact cases exist)
  r1-row0-straddle        lin320: in the wave that straddles M, the residual of     a residual and M % 32 > 8
                          rows + 8 / + 16 / + 24 of a lane comes from row 0
  rv-row0-of-wave         lin320: the row vector of a wave's first row for all 32   a row vector and M > 1
  store-row-M             both: a store to row M                                    every case (the guard row behind the output)
  pos-mod-T               ff320: pos[m % T] instead of pos[(m / HW) % T]            pos with HW > 1
  ln-unrounded            ff320: out_ln normalises the row before its rounding      caught by ff320/d-lnround-M33; WITHIN the
                                                                                    tolerance on Gaussian rows (asserted)"""
import collections

import pytest
import torch

import emu_ops
import l0_cases as lc
import op_cases as oc

CPU_CASES = (list(lc.CASES) + [lc.periodic_lin(inst, N, data, lc.CPU_CUS) for inst, N, data in lc.PERIODIC_LIN]
             + [lc.periodic_ff(kind, lc.CPU_CUS) for kind in lc.PERIODIC_FF])
CAUGHT = collections.defaultdict(list)


def _arg(v):
    return v.cut(v.base) if isinstance(v, oc.View) else v


# ---- the table holds what it is there for ----------------------------------------------------------------------------------
def test_matrix_a_coverage():
    a = [c for c in lc.CASES if c.matrix == "a"]
    assert all(c.op == "lin320" and c.tol == "exact" for c in a)
    assert len(lc.INSTANCES) == 8 and len(set(lc.INSTANCES)) == 8
    for inst in lc.INSTANCES:
        mine = [c for c in a if c.meta["inst"] == inst]
        assert {c.meta["N"] for c in mine} == set(lc.LIN_N) == {64, 128, 192, 256, 320, 384, 960}, inst
        assert {c.meta["M"] for c in mine} == set(lc.LIN_M) == {1, 7, 8, 9, 25, 31, 32, 33, 255, 256, 257, 481, 505}, inst
        if inst[1]:
            assert {c.meta["rvmap"] for c in mine} == {"quirk", "row"}, inst
        assert {c.meta["bias"] for c in mine} == {True, False}, inst
    # the instance a case launches is read off its arguments, as the launcher reads it
    for c in a:
        kw = c.build()
        assert (int(bool(kw.get("norm"))), int("rowvec" in kw), int("r1" in kw)) == c.meta["inst"], c.id
        if "rowvec" in kw:
            assert kw["rv"] == (lc.RV_QUIRK if c.meta["rvmap"] == "quirk" else (1 << 30, 0, lc.RV_ROWS, 1 << 30)), c.id
            assert kw["rowvec"].shape[0] == (5 if c.meta["rvmap"] == "quirk" else lc.RV_ROWS)


def test_matrix_d_and_e_coverage():
    d = [c for c in lc.CASES if c.matrix == "d"]
    for kind in ("plain", "pos", "r2", "ln", "pos+r2+ln"):
        want = tuple(k for k in kind.split("+") if k != "plain")
        assert {c.meta["M"] for c in d if c.meta["kind"] == want} == set(lc.FF_M) == {1, 31, 32, 33, 127, 128, 129, 225}, kind
    assert all(c.meta["HW"] == 7 and c.meta["T"] == 5 for c in d if "pos" in c.meta["kind"])
    assert "ff320/d-lnround-M33" in lc.BY_ID
    e = [c for c in lc.CASES if c.matrix == "e"]
    assert {(c.op, c.meta["M"]) for c in e} == {("lin320", 300), ("ff320", 200)}
    for c in e:
        if c.meta["poison"]:
            row, col, val = c.meta["poison"]
            whole_nan_row = row in (0, c.meta["M"] - 1) and col is None and val != val
            assert whole_nan_row or (row % 32 == 0 and col is not None and val == lc.INF), c.id
    assert {c.meta["poison"][0] for c in e if c.meta["poison"] and c.op == "lin320"} == {0, 299, 32}


def test_periodic_cases_reach_the_ring_phases():
    """at the real grid and at the scaled one: the tile count gives some workgroup a fourth (lin320), a third (ff320) tile, and
    the ring phases g % 3 at which a workgroup's tiles start are all of 0, 1, 2"""
    assert {(i, N) for i, N, _ in lc.PERIODIC_LIN} >= {(i, N) for i in ((0, 0, 0), (1, 0, 0), (0, 1, 1), (1, 1, 1)) for N in (64, 128, 320, 960)}
    assert {d for _, N, d in lc.PERIODIC_LIN if N < 960} == {"exact", "gauss"} and set(lc.PERIODIC_FF) == {"plain", "pos+r2+ln", "r2"}
    for cus in (lc.CPU_CUS, 256, 304):
        for N in (64, 128, 320):
            reps = lc.periodic_reps(256, 3, cus)
            ntiles = -(-reps * lc.P_ROWS // 256)
            assert ntiles >= 3 * cus + 1 and -(-ntiles // cus) >= 4
            assert {(k * (N // 64)) % 3 for k in range(3)} == {0, 1, 2}
        assert -(-lc.periodic_reps(256, 2, cus) * lc.P_ROWS // 256) >= 2 * cus + 1
        assert -(-lc.periodic_reps(128, 2, cus) * lc.P_ROWS // 128) >= 2 * cus + 1
    for c in CPU_CASES:
        if c.matrix in "bc":
            assert c.meta["reps"] >= 2 and c.meta["M"] == c.meta["reps"] * lc.P_ROWS and c.meta["M"] < 4000, c.id
    ff = lc.periodic_ff("pos+r2+ln", lc.CPU_CUS).build()
    assert ff["HW"] == 1 and ff["T"] == lc.P_ROWS and ff["pos"].shape == (lc.P_ROWS, 320)
    lin = lc.periodic_lin((1, 1, 1), 128, "gauss", lc.CPU_CUS).build()
    assert lin["rv"] == (1 << 30, 0, lc.P_ROWS, 1 << 30) and lin["rowvec"].shape == (lc.P_ROWS, 128)


def test_layout_rules():
    """every fp16 2-D argument is a guarded view (NaN rows before and after, 8 NaN columns on the left, ld > width), the leading
    dimensions of one call differ, out / ln_out buffers start as NaN"""
    for c in CPU_CASES:
        kw = c.build()
        flat = {}
        for name, v in kw.items():
            for i, e in enumerate(v if isinstance(v, tuple) else (v,)):
                flat[f"{name}[{i}]" if isinstance(v, tuple) else name] = e
        lds = []
        for name, v in flat.items():
            if not (isinstance(v, oc.View) or torch.is_tensor(v)):
                continue
            t = _arg(v)
            if t.dtype == oc.F16 and t.dim() == 2:
                assert isinstance(v, oc.View), (c.id, name)
                inside = torch.zeros(v.base.shape, dtype=torch.bool)
                v.cut(inside)[...] = True
                assert torch.isnan(v.base[~inside]).all(), (c.id, name)
                r, col = torch.nonzero(inside)[0].tolist()
                assert r >= 1 and col >= 8 and not inside[-1].any() and v.base.shape[1] > col + t.shape[1], (c.id, name)
                lds.append(v.base.shape[1])
                if name in ("out", "ln_out[2]"):
                    assert torch.isnan(t).all(), c.id
        assert len(set(lds)) == len(lds) >= 2, (c.id, lds)


def test_unpacking_equals_the_stand_ins():
    from mofa_video_amd.weights import pack_lin320
    w = oc._h(192, 320, seed=5)
    wp, _ = pack_lin320(w)
    assert torch.equal(lc.unpack_lin320(wp), w) and torch.equal(emu_ops.unpack_lin320(wp), w)
    w1p, _, w2p, _ = lc.ff_params()
    for a, b in zip(lc.unpack_ff320(w1p, w2p), emu_ops.unpack_ff320(w1p, w2p)):
        assert torch.equal(a, b)


# ---- the exact families are exact -------------------------------------------------------------------------------------------
def test_exact_lin320_data_is_on_its_grids_and_rounds_twice():
    shares = []
    for c in CPU_CASES:
        if c.op != "lin320" or c.tol != "exact":
            continue
        kw = c.build()
        x, w = _arg(kw["x"]).double(), lc.unpack_lin320(kw["wp"]).double()
        norm = bool(kw.get("norm"))
        if c.meta.get("poison"):
            continue
        if norm:
            assert bool(((x > 0).sum(1) == 160).all()) and bool((x.abs() == x.abs()[:, :1]).all()), c.id
            assert set(x.abs()[:, 0].tolist()) <= set(lc.LN_AMPS), c.id
            xh = lc.round16(lc.layer_norm64(x, kw["eps"])).double()
            assert bool((xh.abs() == 1).all()) and bool((xh == torch.sign(x)).all()), c.id
            assert bool((w * 128 == (w * 128).round()).all()) and w.abs().max() <= 1, c.id
        else:
            xh = x
            assert bool((x * 16 == (x * 16).round()).all()) and x.abs().max() <= 4, c.id
            assert bool((w * 64 == (w * 64).round()).all()) and w.abs().max() <= 0.5, c.id
        for name in ("bias", "rowvec"):
            if name in kw:
                t = kw[name].double()
                assert bool((t * 1024 == (t * 1024).round()).all()) and t.abs().max() <= (8 if name == "rowvec" or not norm else 176), (c.id, name)
        # every partial sum is one of < 2^24 multiples of 2^-10: the sum of the magnitudes bounds them all
        mag = xh.abs() @ w.abs().T + (kw["bias"].double().abs() if "bias" in kw else 0) + (8 if "rowvec" in kw else 0)
        assert mag.max().item() * 1024 < 2 ** 24, c.id
        for s in (kw["s_acc"], kw.get("s1", 1.0)):
            assert s in (0.25, 0.5, 1.0, 2.0)
        if "r1" in kw:
            r1 = _arg(kw["r1"]).double()
            assert bool((r1 * 64 == (r1 * 64).round()).all()) and r1.abs().max() <= 8, c.id
            rows = min(c.meta["M"] // c.meta["reps"], r1.shape[0])
            acc = xh @ w.T + (kw["bias"].double() if "bias" in kw else 0)
            if "rowvec" in kw:
                acc = acc + kw["rowvec"].double()[lc.rv_index(x.shape[0], kw["rv"])]
            twice = lc.round16(lc.round16(kw["s_acc"] * acc).double() + kw["s1"] * r1)
            once = lc.round16(kw["s_acc"] * acc + kw["s1"] * r1)
            shares.append(((twice != once).sum().item(), twice.numel()))
            assert rows > 0
    # the two rounding orders differ in a good share of the elements: the exact cases tell them apart
    diff, total = sum(s[0] for s in shares), sum(s[1] for s in shares)
    assert diff / total > 0.05, (diff, total)


def test_lnround_case_is_exact():
    kw = lc.BY_ID["ff320/d-lnround-M33"].build()
    x, r2 = _arg(kw["x"]).double(), _arg(kw["r2"]).double()
    assert kw["s_acc"] == 2.0 ** -30 and kw["s1"] == 1.0 and kw["s2"] == 1.0
    y = x + r2
    assert bool((y * 64 == (y * 64).round()).all()) and torch.equal(y.float().double(), y)            # exact in fp32
    assert y.min() >= 256 and y.max() < 1024                                                       # fp16 spacing 0.25 / 0.5
    off = (lc.round16(y).double() - y).abs()
    assert off.max() >= 0.125 and (off > 0).float().mean() > 0.5
    want, _ = lc.ff320_ref({k: (_arg(v) if not isinstance(v, tuple) else tuple(_arg(e) for e in v)) for k, v in kw.items()})
    assert torch.equal(want, y), "f16(s_acc * FF) is not zero"


# ---- the stand-ins pass, the mutants fail -----------------------------------------------------------------------------------
def _checked(module, case):
    r = oc.run(module, case, "cpu")
    worst, errs = lc.check_run(case, r, case.meta["cus"] if case.matrix in "bc" else None)
    return worst, errs, r


def _out_bits(r):
    return [r.placed[n].buf for n in ("out", "ln_out[2]") if n in r.placed]


@pytest.mark.parametrize("case", CPU_CASES, ids=repr)
def test_stand_in_passes_and_the_model_is_the_stand_in(case):
    worst, errs, r = _checked(emu_ops, case)
    assert not errs, errs
    assert worst <= 1.0 and (worst == 0.0 or case.tol != "exact"), (case.id, worst)
    _, merrs, mr = _checked(lc.model(None, lc.CPU_CUS), case)
    assert not merrs, merrs
    for a, b in zip(_out_bits(mr), _out_bits(r)):
        assert oc.same_bits(a, b), f"{case.id}: l0_cases.model(None) is not the stand-in"


@pytest.mark.parametrize("defect", lc.MUTANTS)
def test_mutant_fails_exactly_where_it_must(defect):
    for case in CPU_CASES:
        if case.op not in lc.MUTANT_OPS[defect]:
            continue
        cus = lc.CPU_CUS if case.matrix in "bc" else lc.NO_CUS
        effect = lc.mutant_effect(defect, case, cus)
        _, errs, mr = _checked(lc.model(defect, cus), case)
        if effect == "caught":
            assert errs, f"{case.id}: mutant {defect} passes"
            CAUGHT[defect].append(case.id)
            continue
        assert not errs, (case.id, defect, errs)
        _, _, tr = _checked(lc.model(None, cus), case)
        same = all(oc.same_bits(a, b) for a, b in zip(_out_bits(mr), _out_bits(tr)))
        assert same == (effect == "same"), f"{case.id}: mutant {defect} expected to be '{effect}'"
    by_matrix = collections.Counter(c.split("/")[1][0] for c in CAUGHT[defect])
    print(f"L0-MUTANT {defect}: caught by {len(CAUGHT[defect])} cases {dict(by_matrix)}, e.g. {CAUGHT[defect][:3]}")
    assert CAUGHT[defect], defect
    if defect == "stale-chunk-third-tile":
        assert set(by_matrix) == {"b", "c"}
    if defect == "ln-unrounded":
        assert CAUGHT[defect] == ["ff320/d-lnround-M33"]
    if defect == "single-rounding":
        assert all("-exact-" in c for c in CAUGHT[defect]) and by_matrix["a"] >= 4 * len(lc.LIN_M)


def test_row_isolation_on_the_stand_ins():
    """matrix e as tests/test_l0_matrix_gpu.py runs it: every row but the poisoned one bit-equal to the clean run"""
    for clean in (c for c in lc.CASES if c.matrix == "e" and c.meta["poison"] is None):
        base = oc.run(emu_ops, clean, "cpu")
        for c in lc.CASES:
            if c.matrix == "e" and c.meta["poison"] and c.id.rsplit("-M", 1)[0] == clean.id.rsplit("-M", 1)[0]:
                assert not lc.isolation_errors(c, oc.run(emu_ops, c, "cpu"), base), c.id
