"""The case table of tests/norm_cases.py proven on the CPU before a GPU sees it: the table holds the widths, row edges and launch
regimes it is there for (asserted from the dispatch rules of csrc/norm.hip written out HERE, independently of the helpers the
table uses), each fp64 reference agrees with torch's own layer_norm / group_norm, a correct implementation passes every check --
and every "wrong kernel" mutant FAILS wherever the geometry says it computes something else.  tests/test_norm_matrix_gpu.py runs
the same cases through the HIP kernels.

The mutants (norm_cases.MUTANTS; norm_cases.mutant_differs: True = must fail, False = asserted bit-equal, None = differs by
roundings only, either is accepted):
  ln-mean-drops-tail-vector  the last partly filled lane round left out of the mean     C / 8 no multiple of LPR
  ln-var-counts-padding      zero-filled vectors add mean^2 to the variance             C / 8 < MAXIT * LPR
  ln-one-pass-var            E[x^2] - mean^2 in fp32                                    must fail on the mean-40 cases
  ln-unbiased                divides by C - 1                                           everywhere but constant rows
  ln-rv-rounded              x + rowvec rounded to fp16 before the statistics           row-vector cases of >= 2048 elements
  ln-rv-no-mod               row-vector index without the modulo                        (M - 1) / rv_div >= rv_mod: meets the NaN guard
  ln-rv-div-after-mod        (row % rv_mod) / rv_div                                    wherever that is another index
  ln-skip-last-pass          rows of the last of nrr passes unwritten                   the big cases (nrr >= 2)
  gn-straddle-dropped        a group loses its channels beyond 2048                     C = 2080, 2560
  gn-count-per-frame         element count per frame, not per set                       frames_per_stat > 1
  gn-set-of-frame            frame % sets as the set index                              more than one set of more than one frame
  gn-walk-no-carry           the row walk without ++row on column wrap (same step count) wherever the simulated walk misses a vector
  gn-last-chunk              rows beyond the last full chunk missing from the partials  HW no multiple of the rows per chunk
  gn-silu-first              SiLU before the affine                                     silu cases

The big LayerNorm cases of C = 392 and 648 (25 M and 42 M elements) are not computed here: their shape is asserted, their checker
is the one the C = 8 and C = 64 big cases prove."""
import collections

import pytest
import torch
import torch.nn.functional as F

import aux_cases as ac
import norm_cases as nc
import op_cases as oc

ON_CPU = [c for c in nc.CASES if not c.big or c.meta["C"] <= 64]
LN = [c for c in nc.CASES if c.op == "layer_norm"]
GN = [c for c in nc.CASES if c.op == "group_norm"]
CAUGHT = collections.Counter()


def _arg(v):
    return v.cut(v.base) if isinstance(v, oc.View) else v


# ---- the dispatch rules of csrc/norm.hip, written out independently of norm_cases ---------------------------------------------
LN_INST = {8: (3, 16), 64: (5, 8), 72: (3, 16), 320: (5, 8), 376: (3, 16), 384: (3, 16), 392: (5, 16), 640: (5, 16), 648: (10, 16),
           1280: (10, 16)}
GN_WALK = {32: (64, 0), 96: (21, 4), 160: (12, 16), 224: (9, 4), 960: (2, 16), 1920: (1, 16), 2048: (1, 0), 2080: (0, 256),
           2560: (0, 256), 4096: (0, 256)}


def test_layer_norm_shape_classes():
    for c in LN:
        C, M = c.meta["C"], c.meta["M"]
        CV = C // 8
        inst = (5, 8) if CV <= 40 and CV % 8 == 0 else (3, 16) if CV <= 48 else (5, 16) if CV <= 80 else (10, 16)
        assert inst == LN_INST[C] == nc.ln_inst(C) and CV <= inst[0] * inst[1], c.id
        groups = 256 // inst[1]
        for slots in (256 * 8, 256 * 4, 256):                         # whatever the occupancy of the instantiation
            passes = -(-M // groups)
            nrr = -(-passes // slots)
            grid = -(-passes // nrr)
            assert (nrr >= 2) == c.big, (c.id, slots)
            assert grid * nrr * groups >= M > (grid - 1) * nrr * groups
        if c.big:                                                    # ... the last pass of the last workgroup is 5 rows: `row >= M` breaks
            assert M == 2 * 2048 * groups + groups + 5 and M * C < 50_000_000 and M % groups == 5, c.id
    small = [c for c in LN if not c.big]
    assert {c.meta["C"] for c in small} == set(nc.LN_WIDTHS) == {8, 72, 320, 376, 384, 392, 640, 648, 1280}
    assert sorted(C // 8 for C in nc.LN_WIDTHS) == [1, 9, 40, 47, 48, 49, 80, 81, 160]
    for C in nc.LN_WIDTHS:                                            # every width at every row edge, plain and with a row vector
        G = 256 // LN_INST[C][1]
        assert G == (32 if C == 320 else 16)
        for M in (1, G - 1, G, G + 1, 101):
            forms = {(c.meta["rv"] is not None) for c in small if c.meta["C"] == C and c.meta["M"] == M and c.meta["family"] == "gauss"}
            assert forms == {False, True}, (C, M)
    # both edges of every dispatch branch; the lane tail empty (whole rounds beyond C / 8), partly filled and full
    assert {LN_INST[C] for C in nc.LN_WIDTHS} == {LN_INST[C] for C in nc.LN_BIG_WIDTHS} == {(5, 8), (3, 16), (5, 16), (10, 16)}
    tails = {C: ("full" if (C // 8) % LN_INST[C][1] == 0 else "part", (LN_INST[C][0] * LN_INST[C][1] - C // 8) // LN_INST[C][1]) for C in nc.LN_WIDTHS}
    assert tails == {8: ("part", 2), 72: ("part", 2), 320: ("full", 0), 376: ("part", 0), 384: ("full", 0), 392: ("part", 1),
                     640: ("full", 0), 648: ("part", 4), 1280: ("full", 0)}
    assert [C for C in nc.LN_BIG_WIDTHS] == [64, 8, 392, 648]         # the smallest width of each instantiation
    big = [c for c in LN if c.big]
    assert {(c.meta["C"], c.meta["rv"] is not None) for c in big} == {(C, f) for C in nc.LN_BIG_WIDTHS for f in (False, True)}
    # row-vector index forms: constant, rows of one pass on different vectors, never beyond vector 0, the wrapping (HW, T)
    rvs = {(c.meta["rv"], c.meta["M"]) for c in LN if c.meta["rv"]}
    assert any(rv == (1, 1) for rv, _ in rvs) and any(rv == (7, 5) for rv, _ in rvs) and any(rv == (M + 3, 2) for rv, M in rvs)
    assert ((37, 25), 37 * 25 * 2) in rvs
    assert {c.meta["eps"] for c in LN} == {1e-5, 1e-6}
    assert {c.meta["family"] for c in LN} == {"gauss", "exact", "const", "offset"}
    for c in LN:                                                     # every case in both forms
        twin = [d for d in LN if d.meta["C"] == c.meta["C"] and d.meta["M"] == c.meta["M"] and d.meta["family"] == c.meta["family"]]
        assert {d.meta["rv"] is not None for d in twin} == {False, True}, c.id


def test_group_norm_shape_classes():
    from mofa_video_amd import ops
    assert nc.GN_FUSED_MAX_ENTRIES == ops.GN_FUSED_MAX_ENTRIES
    grid = [c for c in GN if c.meta["family"] == "gauss" and not c.meta["xw"] and (c.meta["HW"] in nc.GN_HW) and c.meta["frames"] in (1, 3)]
    for C in nc.GN_WIDTHS:
        CV = C // 8
        drow = 256 // CV
        assert (drow, 256 - drow * CV) == GN_WALK[C] == nc.gn_walk(C), C
        mine = [c.meta for c in grid if c.meta["C"] == C]
        assert {m["HW"] for m in mine} >= {1, 15, 16, 17, 145}, C     # every width meets every HW edge
        assert {m["frames"] for m in mine} == {1, 3} and {m["silu"] for m in mine} == {False, True}, C
        assert {m["fps"] for m in mine if m["frames"] == 3} == {1, 3}, C
    # the classes of the row walk: several rows per step with and without a column remainder, one row per step with (the decoder
    # concat widths 960 / 1920: remainder 16) and without (2048), and more than 256 vectors per row
    classes = {(min(d, 2), v > 0) for d, v in GN_WALK.values()}
    assert classes == {(2, False), (2, True), (1, True), (1, False), (0, True)} and GN_WALK[960] == (2, 16) and GN_WALK[1920] == (1, 16)
    # gn_partial: idle threads where C / 8 does not divide 256, one or two passes over the columns, a group astride the boundary
    for C, (cols, rl, passes) in {32: (4, 64, 1), 96: (12, 21, 1), 160: (20, 12, 1), 224: (28, 9, 1), 960: (120, 2, 1), 1920: (240, 1, 1),
                                  2048: (256, 1, 1), 2080: (256, 1, 2), 2560: (256, 1, 2), 4096: (256, 1, 2)}.items():
        assert nc.gn_partial_geom(17, C)[:3] == (cols, rl, passes), C
    assert {C for C in nc.GN_WIDTHS if nc.gn_straddles(C)} == {2080, 2560} and (2080 // 32) % 2 == 1 and 2048 % 65 != 0
    assert max(nc.GN_WIDTHS) == 4096
    # chunks of gn_partial: one up to 144 rows, a ragged second at 145
    assert [nc.gn_partial_geom(HW, 32)[3:] for HW in (1, 15, 16, 17, 145)] == [(1, 1), (15, 1), (16, 1), (17, 1), (73, 2)]
    # launch regimes of gn_apply, for any occupancy (1 .. 8 workgroups per CU)
    for wpc in range(1, 9):
        assert nc.gn_rows_per_wg(24, 32, 2304, wg_per_cu=wpc) == 24                      # chunks = 0 -> 1: a workgroup walks its frame
        rpw = nc.gn_rows_per_wg(1000, 32, 64, wg_per_cu=wpc)
        assert rpw >= 32 and (wpc != 8 or (rpw == 32 and 1000 % rpw == 8)), (wpc, rpw)     # (8 = the kernel's own occupancy: ragged)
        for HW in (1, 15, 16):
            assert nc.gn_rows_per_wg(HW, 32, 3, wg_per_cu=wpc) == 16
        assert -(-145 // nc.gn_rows_per_wg(145, 4096, 3, wg_per_cu=wpc)) >= 2           # one row into a later chunk
    ids = {c.id for c in GN}
    assert {"group_norm/one-workgroup-per-frame-f2304-HW24-C32", "group_norm/ragged-last-chunk-f64-HW1000-C32"} <= ids
    # past GN_FUSED_MAX_ENTRIES: gn_finalize + affine_act
    split = [c for c in GN if c.meta["fps"] * nc.gn_nchunks(c.meta["HW"]) > ops.GN_FUSED_MAX_ENTRIES]
    assert [c.id for c in split] == ["group_norm/split-path-f33-fps33-HW2304-C32"]
    assert {(c.meta["C"], c.meta["xw"] > c.meta["C"], c.meta["out_extra"] > 0) for c in GN if c.meta["xw"]} == {(960, True, True), (2080, True, True)}
    assert any(c.meta["fps"] > 1 and c.meta["frames"] // c.meta["fps"] > 1 for c in GN)


def test_row_walk_simulation_covers_every_vector():
    for C in nc.GN_WIDTHS:
        for nrows in (1, 15, 16, 17, 33):
            assert bool(nc.gn_walk_written(nrows, C // 8).all()), (C, nrows)
    assert not bool(nc.gn_walk_written(16, 120, carry=False).all()) and bool(nc.gn_walk_written(16, 256, carry=False).all())


def test_layout_rules():
    """every fp16 argument is a guarded view (NaN rows before and after, 8 NaN columns on the left, ld > width), the leading
    dimensions of one call differ, ``out`` starts as NaN, the row vector lies between NaN rows and fp16 cannot hold its values"""
    for c in ON_CPU:
        kw = c.build()
        lds = []
        for name, v in kw.items():
            if not isinstance(v, oc.View):
                assert not (torch.is_tensor(v) and v.dtype == oc.F16), (c.id, name)
                continue
            t = _arg(v)
            inside = torch.zeros(v.base.shape, dtype=torch.bool)
            v.cut(inside)[...] = True
            assert torch.isnan(v.base[~inside]).all() and inside[0].sum() == 0 and inside[-1].sum() == 0, (c.id, name)
            if t.dtype == oc.F16:
                assert int(torch.nonzero(inside)[0][1]) >= 8 and v.base.shape[1] > t.shape[1], (c.id, name)
                lds.append(v.base.shape[1])
                assert name != "out" or torch.isnan(t).all(), c.id
            else:
                assert name == "rowvec" and t.shape[0] == kw["rv_mod"] and (t.half().float() != t).float().mean() > 0.99, c.id
        assert len(lds) == 2 and len(set(lds)) == 2, (c.id, lds)
        g, b = kw["gamma"].double(), kw["beta"].double()
        assert c.meta["C"] == 8 or (g.std() > 0.5 and b.std() > 0.5), c.id


def test_references_agree_with_torch():
    for c in ON_CPU:
        kw = {k: _arg(v) for k, v in c.build().items()}
        m, C = c.meta, c.meta["C"]
        g, b = kw["gamma"].double(), kw["beta"].double()
        if c.op == "layer_norm":
            v = kw["x"].double()
            if m["rv"]:
                v = v + kw["rowvec"].double()[(torch.arange(m["M"]) // m["rv"][0]) % m["rv"][1]]
            want = F.layer_norm(v, (C,), g, b, m["eps"])
            got = torch.cat([nc.ln_ref(kw["x"][r0:r0 + 8192], kw["gamma"], kw["beta"], m["eps"], kw.get("rowvec"), kw.get("rv_div", 1),
                                       kw.get("rv_mod", 1), r0)[0] for r0 in range(0, m["M"], 8192)])
        else:
            x = kw["x"][:, :C].double()
            nsets = m["frames"] // m["fps"]
            got = nc.gn_ref(kw["x"][:, :C], kw["gamma"], kw["beta"], m["frames"], m["HW"], kw["eps"], m["fps"], m["silu"])[0]
            if m["fps"] * m["HW"] * (C // 32) == 1:                   # one element per group (torch refuses it): y = beta
                assert (got - (F.silu(b) if m["silu"] else b)).abs().max().item() <= 1e-14, c.id
                continue
            want = F.group_norm(x.reshape(nsets, m["fps"] * m["HW"], C).permute(0, 2, 1), 32, g, b, kw["eps"]).permute(0, 2, 1).reshape(-1, C)
            want = F.silu(want) if m["silu"] else want
        scale = float(want.abs().max()) + 1.0
        # (a constant row or a one-element group: rstd = eps^-1/2 multiplies the fp64 rounding of x - mean)
        assert (got - want).abs().max().item() <= 1e-10 * scale, (c.id, (got - want).abs().max().item())


def test_exact_families_lie_on_their_grid_and_are_mostly_tie_free():
    seen = collections.Counter()
    for c in ON_CPU:
        if c.meta["family"] != "exact":
            continue
        kw = {k: _arg(v) for k, v in c.build().items()}
        x = kw["x"][:, :c.meta["C"]].double()
        assert bool((x * 4 == (x * 4).round()).all()) and x.abs().max() <= 6.0, c.id
        w = c.ref(kw)[0]
        assert w.exact.float().mean().item() > (0.9 if c.op == "layer_norm" else 0.5), (c.id, w.exact.float().mean().item())
        seen[c.op] += 1
    assert seen["layer_norm"] >= 2 and seen["group_norm"] >= 2
    c = nc.BY_ID["layer_norm/C8-M17-const"]                          # variance 0 at a power-of-two width: fl16(beta), every element
    kw = {k: _arg(v) for k, v in c.build().items()}
    w = c.ref(kw)[0]
    assert bool(w.exact.all()) and bool((w.ref == kw["beta"].double()).all())


def test_tie_free_means_one_rounding_result():
    g = torch.Generator().manual_seed(5)
    ref = torch.cat([torch.randn(20000, generator=g, dtype=torch.float64) * 3, torch.tensor([1.0, 2.0, -4.0, 0.0, 2.0 ** -15, 1.0 + 2.0 ** -11])])
    b32 = torch.rand(ref.shape, generator=g, dtype=torch.float64) * 2.0 ** -14 * ref.abs().clamp(min=2.0 ** -10)
    b32[-6] = 1.5 * 2.0 ** -12                                       # reaches the tie BELOW 1.0 (half the spacing of the one above)
    free = nc.tie_free(ref, b32)
    assert 0.5 < free.float().mean().item() < 1.0
    for t in (-1.0, -0.5, 0.5, 1.0):
        moved = ac.round16(ref + t * b32)
        assert bool((moved[free] == ac.round16(ref)[free]).all()), t
    assert not free[-1] and not free[-6]                             # a tie itself; 1.0


# ---- a correct implementation passes, the mutants fail ----------------------------------------------------------------------
def _checked(module, case):
    r = oc.run(module, case, "cpu")
    worst, errs = nc.check_run(case, r)
    return worst, errs, r


@pytest.mark.parametrize("case", ON_CPU, ids=repr)
def test_reference_implementation_passes(case):
    truth = nc.impl(None)
    worst, errs, r = _checked(truth, case)
    assert not errs, errs
    assert worst <= 1.0, (case.id, worst)
    if not case.big:
        oc.check_out_is_honoured(truth, case, "cpu", r)


@pytest.mark.parametrize("defect", nc.MUTANTS)
def test_mutant_fails_wherever_it_differs(defect):
    truth = nc.impl(None)
    op = "layer_norm" if defect.startswith("ln-") else "group_norm"
    for case in ON_CPU:
        differs = nc.mutant_differs(defect, case)
        if case.op != op or (case.big and not differs):
            assert case.op == op or differs is False
            continue
        _, errs, mr = _checked(nc.impl(defect), case)
        if differs:
            assert errs, f"{case.id}: mutant {defect} passes"
            CAUGHT[defect] += 1
        elif differs is False:                                       # no defect on this geometry: asserted equal, not skipped
            tr = oc.run(truth, case, "cpu")
            assert not errs, (case.id, defect, errs)
            for (_, a, _), (_, b, _) in zip(mr.outputs(), tr.outputs()):
                assert oc.same_bits(a, b), (case.id, defect)
    print(f"NORM-MUTANT {defect}: caught on {CAUGHT[defect]} cases")
    assert CAUGHT[defect] >= 1, defect


def test_argument_edges_rejected_before_any_device_call():
    """the argument lists tests/test_norm_matrix_gpu.py sends on the GPU, sent here on host buffers first: each returns MOFA_EINVAL
    from the entry point's own checks (there is no device here: a launch attempt would return MOFA_ELAUNCH instead), so on the GPU
    none of them -- C = 0 and C = -32, which six GroupNorm entry points used to accept, among them -- reaches a kernel"""
    from mofa_video_amd import lib as L
    lib = L.load()
    bufs = nc.edge_buffers("cpu")
    snaps = [t.clone() for t in bufs]
    calls = nc.edge_calls(lib, [L.ptr(t) for t in bufs], None)
    assert len(calls) >= 60
    for part in ("layernorm C 0", "layernorm C 1288", "layernorm rv_div 0", "layernorm rv_mod 0", "gn apply C 0", "gn apply C -32", "gn gathered C 0",
                 "gn finalize C -32", "gn reduce C 0", "gn finalize_sums C -32", "gn affine C 0", "gn apply C 40", "gn apply C 4128",
                 "gn finalize HW 0", "gn reduce HW 0", "gn gathered nentries 4097", "gn gathered nentries 0", "gn finalize_sums count_per_group 0",
                 "gn apply nframes % frames_per_stat"):
        assert part in calls, part
    wrong = {name: rc for name, rc in ((name, call()) for name, call in calls.items()) if rc != nc.MOFA_EINVAL}
    assert not wrong, f"accepted (return code): {wrong}"
    for t, s in zip(bufs, snaps):
        assert oc.same_bits(t, s)
