"""The case table of tests/vae_attn_cases.py proven on the CPU before a GPU sees it: the table holds the shapes it is there for,
every exact family's precondition holds, each reference agrees with an independent torch spelling (``torch.softmax`` in fp64,
``reshape`` / ``permute``, ``scaled_dot_product_attention``), a correct implementation passes every check, ``vae.mid_attention_core``
passes them with the stand-ins of tests/emu_ops.py installed (the slicing, the scale and the launch order are host code) -- and
every "wrong kernel" mutant FAILS wherever ``vae_attn_cases.mutant_differs`` says it computes something else and EQUALS the truth
elsewhere.  tests/test_vae_attn_gpu.py runs the same cases through the HIP kernels."""
import collections
import math

import pytest
import torch
import torch.nn.functional as F

import aux_cases as ac
import op_cases as oc
import vae_attn_cases as vc

CAUGHT = collections.Counter()


def _arg(v):
    return v.cut(v.base) if isinstance(v, oc.View) else v


def test_table():
    vc.assert_table()
    assert vc.OPS == ("softmax_rows_", "transpose_v", "mid_attention_core")


def test_layout_rules():
    for c in vc.CASES:
        kw = c.build()
        lds = []
        for name, v in kw.items():
            if not isinstance(v, oc.View):
                assert not torch.is_tensor(v), (c.id, name)
                continue
            t = _arg(v)
            inside = torch.zeros(v.base.shape, dtype=torch.bool)
            v.cut(inside)[...] = True
            assert torch.isnan(v.base[~inside]).all() and not inside[0].any() and not inside[-1].any(), (c.id, name)
            assert v.base.shape[1] % 8 == 0
            if c.op == "softmax_rows_":
                assert (v.base.shape[1] > t.shape[1]) == c.meta["padded"], c.id
            else:
                assert v.base.shape[1] > t.shape[1] and not inside[:, :8].any(), (c.id, name)
            if c.op == "transpose_v":
                assert torch.nonzero(inside)[0].tolist()[1] == 72         # a column block at a non-zero column offset
            lds.append(v.base.shape[1])
        assert len(set(lds)) == len(lds), (c.id, lds)


def test_exact_families_are_exact():
    for c in vc.CASES:
        kw, m = c.build(), c.meta
        if c.op == "softmax_rows_":
            x = _arg(kw["x"])
            hot = vc.hot_columns(m["rows"], m["cols"])
            if m["family"] == "const":
                assert bool((x == x[:, :1]).all()) and set(x[:, 0].tolist()) <= {0.0, 65504.0, -65504.0}
                e = torch.exp(x.float() - x.float().amax(1, keepdim=True))
                assert bool((e == 1).all()) and float(e.sum(1)[0]) == m["cols"]
            elif m["family"] == "onehot":
                assert bool((x[torch.arange(m["rows"]), hot] == 0).all()) and int((x == -vc.INF).sum()) == x.numel() - m["rows"]
            else:
                assert bool((x.float().argmax(1) == torch.tensor(hot)).all()), c.id
                assert bool(((x.float().amax(1, keepdim=True) > x.float()).sum(1) == m["cols"] - 1).all()), c.id
            if m["family"] == "tail" and m["rows"] > 1:
                p = ac.round16(vc.softmax_ref(x.double())[0]).double()
                rest = p.amin(1)
                assert rest.max() >= 2.0 ** -14 or m["cols"] > 4000      # from normal values ...
                assert bool(((rest > 0) & (rest < 2.0 ** -14)).any()) and rest.min() == 0.0, c.id     # ... through subnormals to zero
        if c.op == "transpose_v":
            v = _arg(kw["v"])
            assert bool((v.float().half() == v).all()) and v.abs().max() <= 2048
            blk = v[:min(64, m["S"]), :64].reshape(-1)
            assert blk.unique().numel() == blk.numel(), c.id
        if c.op == "mid_attention_core":
            q, k, v = _arg(kw["q"]), _arg(kw["k"]), _arg(kw["v"])
            S, C, n = m["S"], m["C"], m["frames"]
            if m["family"] == "uniform":
                assert bool((q == 0).all()) and bool((v == v.round()).all()) and v.abs().max() <= 8 and S & (S - 1) == 0
                mean = v.double().reshape(n, S, C).mean(1)
                assert bool((ac.round16(mean).double() == mean).all()), c.id
                assert not bool((mean[0] == mean[1]).all()) and not bool((mean[1] == mean[2]).all())
            if m["family"] == "onehot":
                s = (q.double().reshape(n, S, C) @ k.double().reshape(n, S, C).transpose(1, 2)) / math.sqrt(C)
                pi = torch.stack(vc.perms(S, n))
                assert bool((s.argmax(2) == pi).all()) and bool(((s != 0).sum(2) == 1).all()) and s.max() == 256 / math.sqrt(C)
                p = torch.softmax(ac.round16(s).double(), 2)
                assert bool(((ac.round16(p) == 1).sum(2) == 1).all()) and bool(((ac.round16(p) != 0).sum(2) == 1).all())
                assert not bool((pi[0] == pi[1]).all()) and not bool((k[:S] == k[S:2 * S]).all())
            if m["family"] == "gauss":
                s = (q.double().reshape(n, S, C) @ k.double().reshape(n, S, C).transpose(1, 2)) / math.sqrt(C)
                assert 6.0 <= s.abs().max() <= 16.0, (c.id, s.abs().max())


def test_references_agree_with_torch():
    for c in vc.CASES:
        kw, m = c.build(), c.meta
        args = {k: _arg(v) for k, v in kw.items()}
        want = c.ref(args)[0]
        if c.op == "softmax_rows_":
            y = F.softmax(args["x"].double(), dim=-1)
            if want.bits is not None:
                assert oc.same_bits(ac.round16(y), want.bits), c.id
            else:
                lse = torch.logsumexp(args["x"].double(), 1, keepdim=True)        # another route to the same numbers
                y2 = torch.exp(args["x"].double() - lse)
                assert (y - want.ref).abs().max() == 0 and ((y2 - want.ref).abs() <= 1e-12 * want.ref + 1e-300).all(), c.id
                assert bool((want.bound >= 2.0 ** -25).all())
        elif c.op == "transpose_v":
            n, ncb, S = args["nframes"], args["ncb"], args["S"]
            y = args["v"].reshape(n, S, ncb, 64).permute(0, 2, 3, 1).reshape(n * ncb * 64, S)
            assert oc.same_bits(y.contiguous(), want.bits), c.id
        elif m["family"] == "gauss":
            n, S, C = m["frames"], m["S"], m["C"]
            q, k, v = (args[t].double().reshape(n, S, C) for t in "qkv")
            y = F.scaled_dot_product_attention(q, k, v).reshape(n * S, C)
            assert (y - want.ref).abs().max() <= 1e-12, c.id


# ---- a correct implementation passes, the mutants fail ----------------------------------------------------------------------
def _checked(module, case):
    r = oc.run(module, case, "cpu")
    worst, errs = ac.check_run(case, r)
    return worst, errs, r


@pytest.mark.parametrize("case", vc.CASES, ids=repr)
def test_reference_implementation_passes(case):
    worst, errs, r = _checked(vc.impl(None), case)
    assert not errs, errs
    assert worst <= 1.0, (case.id, worst)


@pytest.mark.parametrize("case", [c for c in vc.CASES if c.op == "mid_attention_core"], ids=repr)
def test_core_passes_on_the_stand_ins(case, monkeypatch):
    """``vae.mid_attention_core`` itself with tests/emu_ops.py installed: its slices, its scale and its launch order"""
    import emu_ops
    emu_ops.install(monkeypatch)
    worst, errs, r = _checked(vc.core_module(), case)
    print(f"VAE-ATTN {case.id} on the stand-ins: worst err / bound {worst:.3f}")
    assert not errs, errs


@pytest.mark.parametrize("defect", vc.MUTANTS)
def test_mutant_fails_wherever_it_differs(defect):
    truth = vc.impl(None)
    for case in vc.CASES:
        if case.op not in vc.MUTANT_OPS[defect]:
            continue
        _, terrs, tr = _checked(truth, case)
        assert not terrs, terrs
        _, errs, mr = _checked(vc.impl(defect), case)
        if vc.mutant_differs(defect, case):
            assert errs, f"{case.id}: mutant {defect} passes"
            CAUGHT[defect] += 1
        else:                                                        # no defect on this geometry: asserted equal, not skipped
            assert not errs, (case.id, defect, errs)
            for (_, a, _), (_, b, _) in zip(mr.outputs(), tr.outputs()):
                assert oc.same_bits(a, b), (case.id, defect)
    print(f"VAE-ATTN-MUTANT {defect}: caught on {CAUGHT[defect]} cases")
    assert CAUGHT[defect] >= 1, defect
