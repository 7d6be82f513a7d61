"""The case table of tests/step_cases.py proven on the CPU before a GPU sees it: the table holds the shapes it is there for, the
exact families are exact, each reference agrees with an independent torch spelling (``permute`` / ``reshape`` for the movers, the
oracle scheduler's ``scale_model_input`` / ``step`` at the tolerances of tests/test_kernels_gpu.py), a correct implementation
passes every check -- and every "wrong kernel" mutant FAILS wherever ``step_cases.mutant_differs`` says it computes something else
and EQUALS the truth elsewhere.  tests/test_step_matrix_gpu.py runs the same cases through the HIP kernels.

The second-pass cases (17 M and 34 M elements) are not computed here: their shape is asserted to exceed the grid cap, their
checker is the one the small cases of the same op prove."""
import collections

import pytest
import torch

import op_cases as oc
import step_cases as sc

SMALL = [c for c in sc.CASES if not c.big]
CAUGHT = collections.Counter()


def _arg(v):
    return v.cut(v.base) if isinstance(v, oc.View) else v


def test_table():
    sc.assert_table()
    assert oc.WRITES["cfg_euler_step_"] == ("latents",) and oc.WRITES["cfg_euler_step_dev_"] == ("latents",)
    from mofa_video_amd import ops
    for c in sc.CASES:                                                # the keyword arguments are those of the entry point
        assert c.op in sc.OPS and hasattr(ops, c.op), c.id


def test_layout_rules():
    """fp16 2-D arguments are views into NaN buffers with guard rows and ld > width (but the ``ld == C`` form, which has no
    buffer of its own), fp32 NCHW tensors lie in a longer NaN buffer, outputs start NaN; ldo = 24 / ldn = 16 as the old test"""
    for c in SMALL:
        kw = c.build()
        for name, v in kw.items():
            if not isinstance(v, oc.View):
                assert not torch.is_tensor(v) or name == "scal", (c.id, name)
                continue
            t = _arg(v)
            inside = torch.zeros(v.base.shape, dtype=torch.bool)
            v.cut(inside)[...] = True
            assert torch.isnan(v.base[~inside]).all(), (c.id, name)
            if t.dtype == oc.F16:
                assert t.dim() == 2 and v.base.shape[1] > t.shape[1] and not inside[0].any() and not inside[-1].any(), (c.id, name)
                assert not inside[:, 0].any(), (c.id, name)
                if name == "out":
                    assert torch.isnan(t).all(), c.id
            else:
                assert t.dim() == 4 and not inside[:5].any() and not inside[-37:].any(), (c.id, name)
        if c.op == "tokens_to_nchw":                                  # the columns >= Cc inside the row hold NaN
            x = _arg(kw["x"])
            assert x.shape[1] > kw["Cc"] and torch.isnan(x[:, kw["Cc"]:]).all() and torch.isfinite(x[:, :kw["Cc"]]).all(), c.id
        if c.op in sc._PREP:
            assert kw["out"].base.shape[1] == 24 and _arg(kw["out"]).shape[1] == 16
        if c.op in sc._EULER:
            assert kw["noise_pred"].base.shape[1] == 16 and _arg(kw["noise_pred"]).shape[1] == 4


def test_exact_families_are_exact():
    for C, HW in ((320, 1000), (65, 65), (1, 1)):
        x = sc.placement(3, C, HW)
        assert bool((x.half().float() == x).all())                   # representable in fp16
        nz = x[0] != 0
        assert int((~nz).sum()) <= -(-C // 64) * -(-HW // 64)         # the one zero of a window
        assert bool((x[0] != x[1])[nz].all()) and bool((x[1] != x[2])[nz].all())     # other values in the next image
        for c0 in range(0, C, 64):
            for p0 in range(0, HW, 64):                               # pairwise distinct inside a 64 x 64 window
                w = x[0, c0:c0 + 64, p0:p0 + 64].reshape(-1)
                assert w.unique().numel() == w.numel(), (C, HW, c0, p0)
        if C >= 128:                                                  # ... in the next channel block, the next pixel block
            assert bool((x[0, :64] != x[0, 64:128])[nz[:64]].all())
        if HW >= 128:
            assert bool((x[0, :, :64] != x[0, :, 64:128])[nz[:, :64]].all())
    for c in SMALL:
        m = c.meta
        if c.op == "nchw_to_tokens" and m["family"] == "R":
            x = _arg(c.build()["x"])
            flat = x.reshape(-1).tolist()
            for v in sc.R_PLANTS[:-1]:
                assert torch.tensor(v).item() in flat, (c.id, v)
            assert int(torch.isnan(x).sum()) == 1 and bool(((x == 0) & torch.signbit(x)).any()), c.id
        if c.op in sc._EULER and m["same_sigma"]:
            kw = c.build()
            s = kw["scal"] if "scal" in kw else None
            assert (s[0] == s[1]) if s is not None else (kw["sigma"] == kw["sigma_next"]), c.id
        if c.op in sc._EULER:
            kw = c.build()
            lat, v = _arg(kw["latents"]), _arg(kw["noise_pred"])
            assert (v.float().abs().mean() > 10 * lat.abs().mean()) == (m["family"] == "V"), c.id
    # the planted values round as the docstring says
    h = sc.n2t_value(torch.tensor([70000.0, -70000.0, 65520.0, 65519.0, 1e-8, 3e-6, -0.0]), 1.0)
    assert h[:4].tolist() == [sc.INF, -sc.INF, sc.INF, 65504.0] and h[4].item() == 0.0 and 0 < h[5].item() < 2.0 ** -14
    assert bool(torch.signbit(h[6]))


def test_references_agree_with_torch():
    from oracle.scheduler import EulerDiscreteScheduler
    sch = EulerDiscreteScheduler()
    sch.set_timesteps(25)
    tab = sc.step_table()
    for c in SMALL:
        kw, m = c.build(), c.meta
        args = {k: _arg(v) for k, v in kw.items()}
        want = c.ref(args)[0]
        if c.op == "nchw_to_tokens":
            x = args["x"]
            n, C = x.shape[:2]
            y = (x * torch.tensor(m["scale"])).permute(0, 2, 3, 1).reshape(-1, C).half()
            got = want.bits[:, :C]
            fin = ~torch.isnan(y)
            assert bool((torch.isnan(got) == torch.isnan(y)).all()) and oc.same_bits(got[fin], y[fin]), c.id
        elif c.op == "tokens_to_nchw":
            n, Cc, H, W = args["n"], args["Cc"], args["H"], args["W"]
            y = args["x"][:, :Cc].reshape(n, H, W, Cc).permute(0, 3, 1, 2).float().contiguous()
            assert oc.same_bits(want.bits, y), c.id
        elif c.op in sc._PREP:
            T, HW, i = m["T"], m["HW"], m["row"]
            lat, img = args["latents"], args["image_latents"]
            sch._step_index = i
            scaled = sch.scale_model_input(lat, sch.timesteps[i]).permute(0, 2, 3, 1).reshape(T * HW, 4)
            l64, im = sc.prepare_ref(lat, img, float(tab[i, 4]), T, HW)
            for half in range(2):
                blk = l64[half * T * HW:(half + 1) * T * HW]
                assert (blk - scaled.double()).abs().max().item() <= 1e-3 * scaled.abs().max().item(), c.id
                ref_img = img[half].permute(1, 2, 0).reshape(HW, 4)
                assert torch.equal(im[half * T * HW:(half + 1) * T * HW].reshape(T, HW, 4), ref_img.expand(T, HW, 4)), c.id
        elif c.op in sc._EULER and not m["same_sigma"]:
            T, HW, i = m["T"], m["HW"], m["row"]
            lat, npred = args["latents"], args["noise_pred"]
            h, w = lat.shape[2:]
            sch._step_index = i
            npf = npred.float().reshape(2, T, h, w, 4).permute(0, 1, 4, 2, 3)
            gs = (torch.linspace(m["gmin"], m["gmax"], T) if T > 1 else torch.tensor([m["gmin"]])).view(T, 1, 1, 1)
            v = npf[0] + gs * (npf[1] - npf[0])
            step = sch.step(v, sch.timesteps[i], lat)
            worst, msg = oc.close_errors(want.ref, step, 1e-5, c.id)
            assert msg is None, msg


# ---- a correct implementation passes, the mutants fail ----------------------------------------------------------------------
def _checked(module, case):
    r = oc.run(module, case, "cpu")
    worst, errs = sc.check_run(case, r)
    return worst, errs, r


@pytest.mark.parametrize("case", SMALL, ids=repr)
def test_reference_implementation_passes(case):
    truth = sc.impl(None)
    worst, errs, r = _checked(truth, case)
    assert not errs, errs
    assert worst <= 1.0, (case.id, worst)
    if case.op == "nchw_to_tokens" and case.meta["family"] == "P":     # (family R holds the infinities and a NaN on purpose)
        oc.check_out_is_honoured(truth, case, "cpu", r)
        assert torch.isfinite(r.ret[:, :case.meta["C"]].float()).all()
    if case.op == "tokens_to_nchw":
        assert torch.isfinite(r.ret).all()


def test_scalar_forms_agree():
    """the host-scalar and the device-scalar form of a step on the same data: latents bit-equal, model input within one fp16 ulp"""
    truth = sc.impl(None)
    for host, dev in sc.pairs():
        a, b = oc.run(truth, host, "cpu").outputs()[0][1], oc.run(truth, dev, "cpu").outputs()[0][1]
        if host.op in sc._EULER:
            assert oc.same_bits(a, b), host.id
        else:
            ulps = (oc.bits(a[:, :4]).int() - oc.bits(b[:, :4]).int()).abs().max().item()
            assert ulps <= 1 and oc.same_bits(a[:, 4:8], b[:, 4:8]), (host.id, ulps)


@pytest.mark.parametrize("defect", sc.MUTANTS)
def test_mutant_fails_wherever_it_differs(defect):
    truth = sc.impl(None)
    for case in SMALL:
        if case.op not in sc.MUTANT_OPS[defect]:
            continue
        _, terrs, tr = _checked(truth, case)
        assert not terrs, terrs
        _, errs, mr = _checked(sc.impl(defect), case)
        if sc.mutant_differs(defect, case):
            assert errs, f"{case.id}: mutant {defect} passes"
            CAUGHT[defect] += 1
            if case.meta.get("family") == "P":
                CAUGHT[defect, "P"] += 1
        else:                                                        # no defect on this geometry: asserted equal, not skipped
            assert not errs, (case.id, defect, errs)
            for (_, a, _), (_, b, _) in zip(mr.outputs(), tr.outputs()):
                nan = torch.isnan(a)
                assert bool((nan == torch.isnan(b)).all()) and oc.same_bits(a[~nan], b[~nan]), (case.id, defect)
    print(f"STEP-MUTANT {defect}: caught on {CAUGHT[defect]} cases")
    assert CAUGHT[defect] >= 1, defect
    if defect in sc.MOVER_MUTANTS and defect != "scale-after-round":
        assert CAUGHT[defect, "P"] >= 1, defect                      # the placement family sees every geometry mutant
