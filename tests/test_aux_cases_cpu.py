"""The case table of tests/aux_cases.py proven on the CPU before a GPU sees it: the table holds the edges it is there for, every
exact family is exact, each fp64 reference agrees with the independent torch spelling of the operation, a correct
implementation passes every check -- and every "wrong kernel" mutant FAILS the check on every case where the geometry says it
computes something else (a checker that cannot fail proves nothing).  tests/test_aux_ops_gpu.py runs the same cases through the
HIP kernels.

The mutants (aux_cases.MUTANTS; aux_cases.mutant_differs states from the geometry alone where each changes the result):
  pool-pad-zero    max pooling counts the padding as 0                    windows that reach into the padding (their maximum is < 0)
  avg-valid-count  the average divides by the number of valid pixels      nowhere: the average takes pad == 0 and floored sizes, every
                                                                          window is whole -- asserted EQUAL on every average case
  ac-false         align_corners=False source coordinates                 an axis with more than one source pixel, resized
  i1-unclamped     i1 = i0 + 1 unclamped: reads the next row              an output pixel ON the last source row / column: the read
                                                                          behind the last image meets the NaN guard, even at weight 0
  no-half-step     bin centres without the half step                      every flow_expectation case
  swap-xy          x and y halves of the logits exchanged                 nbins > 1
  drop-high-half   the bins >= 64 (the ``lane + 64`` half) dropped        nbins > 64
  w-div            w[row // HW] instead of w[row % HW]                    mask_blend with more than one image
  sub-round        subsample with rounding (offset s / 2), not floor      s >= 2
  sigmoid-col1     the matting mask from column 1 of the logit buffer     every matting_blend case

Second-pass cases (33 M elements) are not computed here: their shape is asserted to exceed the grid cap, their checker is the
one the small case of the same op proves."""
import collections

import pytest
import torch
import torch.nn.functional as F

import aux_cases as ac
import op_cases as oc

SMALL = [c for c in ac.CASES if not c.big]
CAUGHT = collections.Counter()


def _nchw(tok, n, H, W):
    return tok.float().reshape(n, H, W, -1).permute(0, 3, 1, 2)


def _tok(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def _arg(v):
    return v.cut(v.base) if isinstance(v, oc.View) else v


# ---- the table holds its edges ---------------------------------------------------------------------------------------------
def test_table_covers_every_op_and_edge():
    assert set(ac.OPS) == {"pool2d", "resize_bilinear_ac", "resize_bilinear_ac_f32", "flow_expectation", "mask_blend", "matting_blend",
                           "geglu", "subsample_tokens", "flow_downscale"}
    by_op = collections.defaultdict(list)
    for c in ac.CASES:
        by_op[c.op].append(c)
    # flow_expectation: every path of the ``lane + 64`` half, a ragged last block, an image boundary inside a block
    assert sorted(c.meta["nbins"] for c in by_op["flow_expectation"]) == [1, 63, 64, 65, 99, 128]
    ntok = ac.FLOW_IMG * ac.FLOW_H * ac.FLOW_W
    assert ntok == 189 and ntok % 4 != 0 and (ac.FLOW_H * ac.FLOW_W) % 4 != 0
    # pooling: every window of the issue's list, odd maps, the production form
    pools = {(c.meta["mode"], c.meta["k"], c.meta["s"], c.meta["p"], c.meta["H"], c.meta["W"]) for c in by_op["pool2d"]}
    for k, s, p in ac.POOL_MAX:
        for H, W in ac.POOL_MAPS:
            assert ("max", k, s, p, H, W) in pools
    assert ("max", 8, 8, 0, 8, 16) in pools and {("avg", 2, 2, 0, 6, 10), ("avg", 2, 2, 0, 7, 9)} <= pools
    assert {c.meta["C"] for c in by_op["pool2d"]} == {8, 64, 320}
    for c in by_op["pool2d"]:                                        # what the entry point accepts (include/mofa_hip.h)
        m = c.meta
        assert m["k"] <= min(m["H"], m["W"]) + 2 * m["p"] and 2 * m["p"] <= m["k"], c.id
    # the resizes: the seven pairs on both, up, down, identity, one-pixel sources and results
    for op in ("resize_bilinear_ac", "resize_bilinear_ac_f32"):
        assert set(ac.RESIZE_PAIRS) <= {c.meta["pair"] for c in by_op[op]}, op
    assert {c.meta["C"] for c in by_op["resize_bilinear_ac"]} == {8, 128}
    assert {c.meta["pair"] for c in by_op["resize_bilinear_ac"] if c.meta["exact"]} == set(ac.RESIZE_EXACT)
    assert any(c.meta["n"] == 6 and c.meta["pair"] == ((4, 6), (8, 12)) for c in by_op["resize_bilinear_ac_f32"])
    # movers
    assert {c.meta["s"] for c in by_op["subsample_tokens"]} == {1, 2, 3, 4}
    fd = by_op["flow_downscale"]
    assert any(c.meta["s"] == 1 for c in fd) and any(c.meta["s"] == c.meta["H"] for c in fd) and any(c.meta["n"] == 1 for c in fd)


def test_second_pass_cases_exceed_the_grid():
    big = [c for c in ac.CASES if c.big]
    assert {c.op for c in big} == {"mask_blend", "matting_blend", "geglu", "subsample_tokens"}
    for c in ac.CASES:
        if "items" in c.meta:
            assert (c.meta["items"] > oc.EW_GRID_ITEMS) == c.big, (c.id, c.meta["items"])
    assert 16400 * (1032 // 8) < oc.EW_GRID_ITEMS               # why the geglu case has 32800 rows (aux_cases docstring)


def test_layout_rules():
    """every fp16 2-D argument but the production-form pool input is a guarded view (NaN rows before and after, 8 NaN columns on
    the left, ld > width), the leading dimensions of one call differ, fp32 NCHW inputs lie in a longer NaN buffer, pure outputs
    start as NaN"""
    for c in SMALL:
        kw = c.build()
        lds = []
        for name, v in kw.items():
            if not (isinstance(v, oc.View) or torch.is_tensor(v)):
                continue
            t = _arg(v)
            if t.dtype == oc.F16 and t.dim() == 2:
                if c.id.endswith("-ld320"):
                    assert t.is_contiguous() and t.shape[1] == 320
                    continue
                assert isinstance(v, oc.View), (c.id, name)
                inside = torch.zeros(v.base.shape, dtype=torch.bool)
                v.cut(inside)[...] = True
                assert torch.isnan(v.base[~inside]).all(), (c.id, name)
                r, col = torch.nonzero(inside)[0].tolist()
                assert r >= 1 and col >= 8 and not inside[-1].any() and v.base.shape[1] > t.shape[1], (c.id, name)
                lds.append(v.base.shape[1])
                if name == "out":
                    assert torch.isnan(t).all(), c.id
            elif t.dtype == oc.F32 and t.dim() == 4:
                assert isinstance(v, oc.View) and torch.isnan(v.base[:5]).all() and torch.isnan(v.base[-37:]).all(), (c.id, name)
        assert len(set(lds)) == len(lds), (c.id, lds)


def test_exact_families_are_exact():
    for c in SMALL:
        kw, m = c.build(), c.meta
        if c.op == "pool2d" and m["mode"] == "avg" and m["data"] == "grid":
            x = _arg(kw["x"])
            assert bool((x.double() * 64 == (x.double() * 64).round()).all()) and x.abs().max() <= 8
            v = x.float().reshape(m["n"], m["H"], m["W"], -1)
            Ho, Wo = ac.pool_size(m["H"], 2, 2, 0), ac.pool_size(m["W"], 2, 2, 0)
            s32 = torch.zeros(m["n"], Ho, Wo, v.shape[-1])
            for ky in range(2):
                for kx in range(2):                                   # the kernel's order: fp32 running sum, then * fl(1 / 4)
                    s32 = s32 + v[:, ky:ky + 2 * Ho - 1:2, kx:kx + 2 * Wo - 1:2]
            got = (s32 * torch.tensor(1.0 / 4)).reshape(-1, v.shape[-1])
            assert bool((got.double() == ac.pool_ref(x.double(), m["n"], m["H"], m["W"], 2, 2, 0, "avg")).all()), c.id
        if c.op == "resize_bilinear_ac" and m["exact"]:
            (Hin, Win), (Hout, Wout) = m["pair"]
            x = _arg(kw["x"])
            assert ac.bilinear_fp32_is_exact(x.double(), m["n"], Hin, Win, Hout, Wout), c.id
            for n_in, n_out in ((Hin, Hout), (Win, Wout)):
                f = ac.ac_coords(n_in, n_out)[1]
                assert bool((f * 4 == (f * 4).round()).all()), c.id
            if (Hin, Win) == (Hout, Wout):                            # the identity returns the input bits
                assert oc.same_bits(c.ref({"x": x})[0].bits, x.contiguous()), c.id


def test_max_pool_border_windows_are_negative():
    """... so a kernel that counted the padding as 0 shows in every one of them; the +65504 entries sit in no such window"""
    seen = 0
    for c in SMALL:
        m = c.meta
        if c.op != "pool2d" or m["mode"] != "max":
            continue
        x = _arg(c.build()["x"])
        assert int((x == 65504).sum()) == 2 and int((x == -65504).sum()) >= 2 and x[x != 65504].max() < 0, c.id
        border = ac.border_windows(m["H"], m["W"], m["k"], m["s"], m["p"])
        y = ac.pool_ref(x.double(), m["n"], m["H"], m["W"], m["k"], m["s"], m["p"], "max").reshape(m["n"], *border.shape, -1)
        assert bool((y[:, border] < 0).all()), c.id
        assert bool(border.any()) == (m["p"] > 0), c.id
        seen += int(border.any())
    assert seen == 3


def test_special_values_are_in_the_data():
    kw = ac.BY_ID["matting_blend/small"].build()
    l = _arg(kw["logit"])
    assert l.shape[1] == 8 and {0.0, 12.0, -12.0, 65504.0, -65504.0} <= set(l[:, 0].tolist())
    assert bool((l[:, 0] != l[:, 1]).any())
    w = ac.BY_ID["mask_blend/small"].build()["w"]
    assert int((w == 0).sum()) == 2 and int((w == 1).sum()) == 2 and w.numel() == 35
    x = _arg(ac.BY_ID["geglu/small"].build()["x"])
    g = x[:, 128:]
    assert {30.0, -30.0, 6.0, -6.0, 0.0} <= set(g.flatten().tolist()) and bool(((g == 0) & torch.signbit(g)).any())
    over = ac.BY_ID["geglu/overflow"]
    want = over.ref({"x": _arg(over.build()["x"])})[0]
    assert int(want.inf.sum()) == 2 and sorted(want.ref[want.inf].tolist()) == [-ac.INF, ac.INF]
    for nb in ac.NBINS:
        l = _arg(ac.BY_ID[f"flow_expectation/nbins{nb}"].build()["logits"])
        assert l.shape == (189, 2 * nb) and bool((l == 65504).any()) and bool((l == -65504).any()) and bool((l == 40).any())
        e0, e1 = ac.FLOW_ROWS["equal"]
        assert bool((l[e0:e1] == l[e0:e1, :1]).all())


# ---- the references against the independent torch spelling ------------------------------------------------------------------
def test_references_agree_with_torch():
    from oracle.cmp import Fuser
    for c in SMALL:
        kw, m = c.build(), c.meta
        args = {k: _arg(v) for k, v in kw.items()}
        want = c.ref(args)[0]
        if c.op == "pool2d":
            n, H, W, C = m["n"], m["H"], m["W"], m["C"]
            x = _nchw(args["x"][:, :C], n, H, W)
            if m["mode"] == "max":
                y = F.max_pool2d(x, m["k"], m["s"], m["p"])
            elif m["data"] == "grid":
                y = F.avg_pool2d(x, m["k"], m["s"])
            else:
                continue
            assert tuple(y.shape[2:]) == (ac.pool_size(H, m["k"], m["s"], m["p"]), ac.pool_size(W, m["k"], m["s"], m["p"])), c.id
            assert oc.same_bits(_tok(y).half(), want.bits), c.id
        elif c.op in ("resize_bilinear_ac", "resize_bilinear_ac_f32"):
            (Hin, Win), (Hout, Wout) = m["pair"]
            x = args["x"].double()
            x4 = _nchw(x, m["n"], Hin, Win).double() if c.op == "resize_bilinear_ac" else x
            y = F.interpolate(x4, size=(Hout, Wout), mode="bilinear", align_corners=True)
            ref = ac.bilinear_ref((_tok(x4) if c.op == "resize_bilinear_ac" else x4.reshape(-1, 1)), m["n"], Hin, Win, Hout, Wout)[0]
            y = _tok(y) if c.op == "resize_bilinear_ac" else y.reshape(-1, 1)
            # rounding the coordinate to fp32 moves it by at most 2^-24 * in, the blend by that times the pixel differences
            assert (y - ref).abs().max().item() <= 2.0 ** -22 * (Hin + Win) * x.abs().max().item(), c.id
        elif c.op == "flow_expectation":
            nb = m["nbins"]
            l = _nchw(args["logits"], ac.FLOW_IMG, ac.FLOW_H, ac.FLOW_W)
            y = Fuser(nb, ac.FMAX).convert_flow(l)
            assert (y.double() - want.ref).abs().max().item() <= 64 * ac.U32 * ac.FMAX, c.id
        elif c.op == "subsample_tokens":
            n, H, W, s = args["n"], args["H"], args["W"], args["s"]
            y = F.interpolate(_nchw(args["x"], n, H, W), scale_factor=1 / s)
            assert oc.same_bits(_tok(y).half(), want.bits), c.id
        elif c.op == "flow_downscale":
            s = args["s"]
            assert oc.same_bits((F.interpolate(args["flow"], scale_factor=1 / s) / s).contiguous(), want.bits), c.id
        elif c.op == "geglu":
            x = args["x"].double()
            y = x[:, :128] * F.gelu(x[:, 128:])
            fin = ~want.inf
            assert (y - want.ref)[fin].abs().max().item() <= 1e-12 * max(1.0, y[fin].abs().max().item()), c.id
        elif c.op == "mask_blend":
            a, b, w = args["a"].double(), args["b"].double(), args["w"].double()
            y = torch.lerp(b.reshape(6, 35, -1), a.reshape(6, 35, -1), w[None, :, None].expand(6, 35, 64)).reshape(210, 64)
            assert (y - want.ref).abs().max().item() <= 1e-12, c.id
        elif c.op == "matting_blend":
            m_ = 1 / (1 + torch.exp(-args["logit"][:, 0].double()))
            y = args["warped"].double() * m_[:, None] + args["matting"].double() * (1 - m_[:, None])
            assert (y - want.ref).abs().max().item() <= 1e-12, c.id


# ---- a correct implementation passes, the mutants fail ----------------------------------------------------------------------
def _checked(module, case):
    r = oc.run(module, case, "cpu")
    worst, errs = ac.check_run(case, r)
    return worst, errs, r


@pytest.mark.parametrize("case", SMALL, ids=repr)
def test_reference_implementation_passes(case):
    truth = ac.impl(None)
    worst, errs, r = _checked(truth, case)
    assert not errs, errs
    # the reference rounded once: half an fp16 ulp, which IS u16 |ref| just above a power of two -- so fp16 outputs may sit near
    # 1.0 of their bound by the final rounding alone; fp32 outputs are rounded 2^13 times finer
    assert worst <= 1.0, (case.id, worst)
    oc.check_out_is_honoured(truth, case, "cpu", r)


@pytest.mark.parametrize("defect", ac.MUTANTS)
def test_mutant_fails_wherever_it_differs(defect):
    truth = ac.impl(None)
    for case in SMALL:
        if case.op not in ac.MUTANT_OPS[defect]:
            continue
        _, terrs, tr = _checked(truth, case)
        assert not terrs, terrs
        _, errs, mr = _checked(ac.impl(defect), case)
        if ac.mutant_differs(defect, case):
            assert errs, f"{case.id}: mutant {defect} passes"
            CAUGHT[defect] += 1
        else:                                                        # no defect on this geometry: asserted equal, not skipped
            assert not errs, (case.id, defect, errs)
            for (_, a, _), (_, b, _) in zip(mr.outputs(), tr.outputs()):
                assert (a is b) or (not torch.is_tensor(a) and a == b) or oc.same_bits(a, b), (case.id, defect)
    print(f"AUX-MUTANT {defect}: caught on {CAUGHT[defect]} cases")
    if defect == "avg-valid-count":
        assert CAUGHT[defect] == 0 and sum(c.op == "pool2d" and c.meta["mode"] == "avg" for c in SMALL) == 4
    else:
        assert CAUGHT[defect] >= 1, defect
