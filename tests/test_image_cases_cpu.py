"""The case table of tests/image_cases.py proven on the CPU before a GPU sees it: the table holds the geometry classes it is there
for (ragged last block, second pass of the flow maximum, largest legal reflection, one-pixel axes, the k1 wrap, rad > 1), every
exact family is exact, the fragile-byte conditions of the flow comparison hold for the chosen seeds, each reference agrees with
torch's CPU op and with ``oracle/``, a correct implementation passes every check -- and every "wrong kernel" mutant FAILS the
check on exactly the cases where ``image_cases.mutant_differs`` says it computes something else.  tests/test_image_ops_gpu.py
runs the same cases through the HIP kernels.

The mutants (image_cases.MUTANTS):
  reflect-symmetric      reflection that repeats the edge pixel (index -1 -> 0)      k > 1
  front-rear-swapped     the longer half of an even window in front                  even k
  axis-swapped           the filter runs along the other axis                        k > 1
  cubic-A-0.5            Keys' A = -0.5                                              some t != 0
  bicubic-ac-false       align_corners=False coordinates                             an axis with more than one source pixel, resized
  taps-unclamped         tap indices not clamped: reads the NaN guard                every case (output pixel 0 reads index -1)
  s-not-rounded          t from the exact product scale * o (a fused multiply)       the 256- and 4097-pixel axes (image_cases docstring)
  patch-px-py-swapped    px and py exchanged inside the patch                        p > 1
  patch-channel-last     columns ordered (py, px, c)                                 p > 1 and C > 1
  nearest-exact-ratio    floor(o * in / out) in integers                             where the index vectors differ (the sweep: anywhere)
  nearest-round          round instead of floor                                      where the index vectors differ
  maxrad-first-pass      the maximum ignores pixels beyond 1024 * 256                the maximum lies beyond them
  maxrad-whole-blocks    the maximum ignores the ragged last block                   the maximum lies in it
  no-k1-wrap             k1 = 56 reads behind the colour wheel                       a pixel at the angle +pi exactly
  unknown-counts-in-max  unknown pixels take part in the maximum                     an unknown pixel is the largest
  nan-not-black          a NaN pixel is coloured                                     the NaN cases
  post-nan-to-zero       the clamp turns NaN into 0                                  the two float modes"""
import collections
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import image_cases as ic
import op_cases as oc

CAUGHT = collections.Counter()
BY_OP = collections.defaultdict(list)
for _c in ic.CASES:
    BY_OP[_c.op].append(_c)


def _arg(v):
    return v.cut(v.base) if isinstance(v, oc.View) else v


def _args(case):
    return {k: _arg(v) for k, v in case.build().items()}


# ---- the table holds its edges ---------------------------------------------------------------------------------------------
def test_table_covers_every_op_and_geometry_class():
    assert set(ic.OPS) == {"filter1d_reflect", "resize_bicubic_ac", "patchify", "resize_nearest_f32", "frames_postprocess", "flow_to_image"}
    assert set(ic.MUTANT_OPS) == set(ic.MUTANTS) and {op for ops in ic.MUTANT_OPS.values() for op in ops} == set(ic.OPS)
    for op in ic.OPS:                                                # a ragged last block behind at least one full one, and less than a wave
        items = [c.meta["items"] for c in BY_OP[op]]
        assert any(i > 256 and i % 256 for i in items), op
    assert any(c.meta["items"] < 64 for c in BY_OP["flow_to_image"]) and any(c.meta["items"] == 1 for c in BY_OP["flow_to_image"])
    fl = {(c.meta["k"], c.meta["axis"], c.meta["H"], c.meta["W"]): c for c in BY_OP["filter1d_reflect"]}
    for key in ((1, 0, 5, 9), (1, 1, 5, 9), (3, 0, 5, 9), (3, 1, 5, 9), (7, 0, 5, 9), (7, 1, 5, 9), (4, 0, 5, 9), (4, 1, 5, 9),
                (7, 1, 3, 4), (5, 0, 3, 4), (6, 1, 3, 4), (6, 0, 4, 3), (3, 1, 1, 9), (3, 0, 9, 1), (5, 1, 11, 13), (4, 0, 11, 13)):
        assert key in fl, key
    largest = [c for c in BY_OP["filter1d_reflect"] if c.meta["rear"] == c.meta["size"] - 1]
    assert {(c.meta["k"] % 2, c.meta["axis"]) for c in largest} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for c in BY_OP["filter1d_reflect"]:                              # what the entry point accepts
        assert c.meta["rear"] < c.meta["size"], c.id
    taps = ic.production_taps()
    assert sorted(taps) == [3, 7]
    prod = [c for c in BY_OP["filter1d_reflect"] if c.meta["kind"] == "production"]
    assert {c.meta["k"] for c in prod} == {3, 7} and any(2 * c.meta["rear"] > c.meta["size"] for c in prod)
    assert {c.meta["kind"] for c in BY_OP["filter1d_reflect"]} == {"copy", "gauss", "exact", "production"}
    pairs = {c.meta["pair"] for c in BY_OP["resize_bicubic_ac"]}
    assert {((1, 1), (4, 6)), ((3, 5), (1, 1)), ((5, 7), (5, 7)), ((3, 5), (9, 17)), ((2, 3), (16, 24)), ((16, 24), (4, 6)),
            ((11, 13), (7, 19)), ((256, 4), (100, 9))} <= pairs
    assert [c.meta["pair"] for c in BY_OP["resize_bicubic_ac"] if c.meta["exact"]] == [ic.BICUBIC_EXACT]
    i0 = ic.cubic_coords(2, 16)[0]                                   # the upscale where all four taps clamp
    assert bool(((i0 - 1 < 0) | (i0 + 2 > 1)).all())
    assert {c.meta["shape"] for c in BY_OP["patchify"]} == {(2, 3, 28, 42, 14, 640), (2, 3, 28, 42, 14, 588), (1, 3, 14, 14, 14, 592),
                                                            (2, 5, 6, 9, 1, 8), (2, 3, 8, 12, 2, 16)}
    sizes = {c.meta["sizes"] for c in BY_OP["resize_nearest_f32"]}
    assert sum(s[:2] == (48, 80) for s in sizes) == 4
    covered = {(H, h) for H, W, h, w in ic.NEAREST_SWEEP} | {(W, w) for H, W, h, w in ic.NEAREST_SWEEP}
    assert covered == {(i, o) for i in range(1, 25) for o in range(1, 25)}
    assert {(c.meta["mode"], c.meta["items"]) for c in BY_OP["frames_postprocess"]} == {(m, n) for m in (0, 1, 2) for n in (70, 1152)}
    # flow: the sizes, the position of the maximum in turn, the second pass
    flows = BY_OP["flow_to_image"]
    assert {(c.meta["H"], c.meta["W"]) for c in flows} >= {(1, 1), (7, 9), (1, 257), (48, 64), (513, 512)}
    assert 513 * 512 > ic.FIRST_PASS and (513 * 512) % 256 == 0
    for (H, W), positions in ic.FLOW_MAX_POSITIONS.items():
        n = H * W
        got = {c.meta["maxpos"] for c in flows if (c.meta["H"], c.meta["W"]) == (H, W) and c.meta["kind"] == "gauss"}
        assert got == {(p,) for p in positions}, (H, W)
        assert {0, n - 1} <= set(positions) and any(p % 256 == 255 and p < n // 256 * 256 for p in positions)
        if n % 256 and n > 256:
            assert n // 256 * 256 in positions and n // 256 * 256 - 1 in positions
        if n > ic.FIRST_PASS:
            assert ic.FIRST_PASS in positions and ic.FIRST_PASS - 1 in positions
    assert sum(c.big for c in flows) == 5 and all((c.meta["n"] > ic.FIRST_PASS) == c.big for c in flows)
    assert {c.meta["kind"] for c in flows} == {"gauss", "axes", "radgt1", "unknown", "exact-1e7", "nan", "all-unknown", "zero", "tiny"}


def test_layout_rules():
    """every tensor argument is a view into a longer buffer: NaN around the inputs, NaN (0xA5 for uint8) in and around ``out``,
    the workspace exactly WS_BYTES inside 0xA5 bytes"""
    for c in ic.CASES:
        if c.big and c.meta["maxpos"] != (0,):
            continue
        for name, v in c.build().items():
            if not isinstance(v, oc.View):
                assert not torch.is_tensor(v), (c.id, name)
                continue
            inside = torch.zeros(v.base.shape, dtype=torch.bool)
            v.cut(inside)[...] = True
            assert v.base.dim() == 1 and inside[0].item() is False and inside[-1].item() is False, (c.id, name)
            first, count = int(torch.nonzero(inside)[0]), int(inside.sum())
            assert first >= 3 and v.base.numel() - first - count >= 11 and v.cut(v.base).is_contiguous(), (c.id, name)
            if v.base.dtype == ic.U8:
                assert bool((v.base == ic.CANARY).all()), (c.id, name)
            elif name == "out":
                assert bool(torch.isnan(v.base).all()), (c.id, name)
            else:
                assert bool(torch.isnan(v.base[~inside]).all()) and not bool(torch.isnan(v.base[inside]).all()), (c.id, name)
            if name == "ws":
                assert count == ic.WS_BYTES and first % 16 == 0


def test_exact_families_are_exact():
    seen = collections.Counter()
    for c in BY_OP["filter1d_reflect"]:
        a = _args(c)
        if c.meta["kind"] == "exact":
            x, taps = a["x"], a["taps"]
            assert bool((x * 64 == (x * 64).round()).all()) and x.abs().max() <= 8 and bool((taps * 8 == (taps * 8).round()).all())
            assert ic.filter_fp32_is_exact(x, taps, a["axis"]), c.id
            seen["filter"] += 1
        elif c.meta["kind"] == "copy":
            assert a["taps"].tolist() == [1.0] and not bool(((a["x"] == 0) & torch.signbit(a["x"])).any())
    for c in BY_OP["resize_bicubic_ac"]:
        (Hin, Win), (Hout, Wout) = c.meta["pair"]
        x = _args(c)["x"]
        if c.meta["exact"]:
            assert bool((x * 4 == (x * 4).round()).all()) and x.abs().max() <= 8
            for n_in, n_out in ((Hin, Hout), (Win, Wout)):
                t = ic.cubic_coords(n_in, n_out)[1]
                assert bool((t * 4 == (t * 4).round()).all()), c.id
            assert ic.bicubic_fp32_is_exact(x.reshape(-1, Hin, Win), Hout, Wout), c.id
            # ... and the 2^-6 grid would not do: the fp32 order rounds there
            assert not ic.bicubic_fp32_is_exact(ic._grid(6, Hin, Win, seed=5, step=64), Hout, Wout)
            seen["bicubic"] += 1
        if (Hin, Win) == (Hout, Wout):                               # the identity: weights exactly (0, 1, 0, 0)
            for n in (Hin, Win):
                i0, t = ic.cubic_coords(n, n)
                assert bool((t == 0).all()) and i0.tolist() == list(range(n))
            assert ic.cubic_weights(torch.zeros(1, dtype=torch.float32)).tolist() == [[0.0, 1.0, 0.0, 0.0]]
            seen["identity"] += 1
    assert seen == {"filter": 4, "bicubic": 1, "identity": 1}


def test_special_values_are_in_the_data():
    for c in BY_OP["patchify"]:
        a = _args(c)
        x, want = a["x"], c.ref(a).bits
        for v in ic.PATCH_PLANTS:
            assert bool(((x == v) & (torch.signbit(x) == (np.signbit(v).item()))).any()), (c.id, v)
        n, C, H, W, p, ld = c.meta["shape"]
        data = want[:, :C * p * p].float()
        assert int(torch.isinf(data).sum()) == 3 and bool((data == 65504).any())
        sub = (data != 0) & (data.abs() < 2.0 ** -14)
        assert bool(sub.any()) and bool(((data == 0) & torch.signbit(data)).any())
        assert int((data == 0).sum()) >= 2                           # 1e-8 -> +0, and the planted -0
        assert oc.same_bits(want[:, C * p * p:], torch.zeros(want.shape[0], ld - C * p * p, dtype=torch.float16))
    for c in BY_OP["frames_postprocess"]:
        x = _args(c)["frames"]
        for v in ic.POST_PLANTS:
            assert bool(((x == v) & (torch.signbit(x) == (np.signbit(v).item()))).any()), (c.id, v)
        assert int(torch.isnan(x).sum()) == 3 * x.shape[0]
        s = (x / 2 + 0.5).clamp(0, 1) * 255                          # the fp32 product the rounding sees: exact ties, even and odd
        tie = s[(s - s.floor()) == 0.5].floor()
        assert bool((tie % 2 == 0).any()) and bool((tie % 2 == 1).any()), c.id
    axes = _args(ic.BY_ID["flow_to_image/axes-7x9-s0"])["flow"].reshape(-1, 2)
    u, v = axes[:, 0], axes[:, 1]
    assert bool(((v == 0) & torch.signbit(v) & (u > 0)).any()) and bool(((u == 0) & torch.signbit(u)).any())
    un, vn, _ = ic.flow_normalised(axes.reshape(7, 9, 2))
    a = (np.arctan2(-vn, -un) / np.pi).astype(np.float32)
    fk = ic._fk(a).reshape(-1)[:56]
    assert set(np.unique(fk).tolist()) == {1.0, 14.5, 28.0, 41.5, 55.0}
    for H, W in ((7, 9), (23, 31)):
        n = H * W
        unk = ic.flow_data("unknown", H, W, 0).reshape(-1, 2)
        assert bool(torch.isinf(unk).any()) and bool((unk == 2e7).any()) and bool((unk == -2e7).any())
        e7 = ic.flow_data("exact-1e7", H, W, 0).reshape(-1, 2)
        r = ic.radius(e7.reshape(H, W, 2))
        assert bool((e7.abs() == 1e7).any(1)[r == r.max()].all()) and r.max() > 1e7     # the largest pixel holds exactly 1e7, known
        nan = ic.flow_data("nan", H, W, 0, n - 3).reshape(-1, 2)
        kinds = {(bool(torch.isnan(p[0])), bool(torch.isnan(p[1]))) for p in nan[torch.isnan(nan).any(1)]}
        assert kinds == {(True, False), (False, True), (True, True)}
        assert torch.nan_to_num(nan, nan=0.0).abs().max() == 1e3       # beside a NaN lies the largest number of the map
    assert bool(torch.isinf(ic.flow_data("all-unknown", 7, 9, 0)).any())
    assert ic.flow_data("tiny", 7, 9, 0).abs().max() < 1e-19


def test_rad_above_one_branch_is_taken():
    """the maximum pixel of the radgt1 cases normalises to an fp32 radius above 1: in the REFERENCE at least one pixel takes
    compute_color's ``col *= 0.75`` branch"""
    p = ic.radgt1_direction()
    for c in BY_OP["flow_to_image"]:
        flow = _args(c)["flow"] if not c.big else None
        if flow is None:
            continue
        un, vn, _ = ic.flow_normalised(flow)
        above = np.sqrt(un ** 2 + vn ** 2) > 1
        if c.meta["kind"] == "radgt1":
            assert above.sum() >= 1 and bool((flow.reshape(-1, 2)[c.meta["maxpos"][0]] == p).all()), c.id
            from oracle.output import flow_to_image
            img = flow_to_image(flow)
            pix = img.reshape(-1, 3)[c.meta["maxpos"][0]]
            assert pix.max() <= 191                                  # floor(255 * 0.75 * col), col <= 1
            assert bool((torch.from_numpy(img) == ic.flow_ref(flow)).all())


# ---- the references against torch's CPU ops and oracle/ ---------------------------------------------------------------------
def test_filter_reference_agrees_with_torch():
    for c in BY_OP["filter1d_reflect"]:
        a = _args(c)
        x, taps, axis, k = a["x"].double(), a["taps"].double(), a["axis"], c.meta["k"]
        front, rear = (k - 1) // 2, k - 1 - (k - 1) // 2
        H, W = x.shape[-2:]
        pad = (front, rear, 0, 0) if axis == 1 else (0, 0, front, rear)
        xp = F.pad(x.reshape(-1, 1, H, W), pad, mode="reflect")
        w = taps.reshape(1, 1, 1, k) if axis == 1 else taps.reshape(1, 1, k, 1)
        y = F.conv2d(xp, w).reshape(x.shape)
        want = c.ref(a)
        ref = want.bits.double() if want.bits is not None else want.ref
        tol = 1e-12 if want.bits is None else 2.0 ** -22 * float(x.abs().max())
        assert tuple(y.shape) == tuple(ref.shape) and (y - ref).abs().max().item() <= tol, c.id


def test_bicubic_reference_agrees_with_aten_within_the_bound():
    worst = 0.0
    for c in BY_OP["resize_bicubic_ac"]:
        a = _args(c)
        (Hin, Win), (Hout, Wout) = c.meta["pair"]
        x = a["x"]
        y = F.interpolate(x, size=(Hout, Wout), mode="bicubic", align_corners=True)
        ratio, errs = ic.check_out(c.id, y, c.ref(a))
        print(f"IMG-ATEN {c.id}: worst err / bound {ratio:.3f}")
        worst = max(worst, ratio)
        assert not errs, errs
    print(f"IMG-ATEN-WORST resize_bicubic_ac: {worst:.3f}")


def test_patchify_and_postprocess_references_agree_with_torch_and_oracle():
    from oracle.output import postprocess
    for c in BY_OP["patchify"]:
        a = _args(c)
        n, C, H, W, p, ld = c.meta["shape"]
        with np.errstate(over="ignore"):
            y = F.unfold(a["x"], kernel_size=p, stride=p).transpose(1, 2).reshape(-1, C * p * p).to(torch.float16)
        assert oc.same_bits(y, c.ref(a).bits[:, :C * p * p].contiguous()), c.id
    for c in BY_OP["frames_postprocess"]:
        a = _args(c)
        x, mode, want = a["frames"], c.meta["mode"], c.ref(a).bits
        if mode == 0:
            got = postprocess(x, "pt")
        else:
            got = torch.from_numpy(postprocess(x, "np"))
            if mode == 2:                                            # numpy_to_pil's own expression; a NaN has no uint8: left out
                nan = torch.isnan(got)
                with np.errstate(invalid="ignore"):
                    got = torch.from_numpy((got.numpy() * 255).round().astype("uint8"))
                assert bool((want[nan] == 0).all())
                got[nan] = 0
        if mode == 2:
            assert bool((got == want).all()), c.id
        else:
            assert bool((torch.isnan(got) == torch.isnan(want)).all()) and int(torch.isnan(want).sum()) == 3 * x.shape[0], c.id
            assert oc.same_bits(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want, nan=0.0)), c.id


def test_nearest_rule_agrees_with_torch_over_the_sweep():
    """the fp32 floor(o * (in / out)) rule against F.interpolate on every (in, out) pair of 1..24 and on the table's cases; the
    two wrong rules differ exactly where their index vectors do -- and somewhere in the sweep"""
    shapes = list(ic.NEAREST_SWEEP) + [c.meta["sizes"] for c in BY_OP["resize_nearest_f32"]]
    differ = collections.Counter()
    for j, (H, W, h, w) in enumerate(shapes):
        x = ic.nearest_data(2, H, W, 1000 + j)
        want = F.interpolate(x[None], size=(h, w), mode="nearest")[0]
        assert oc.same_bits(ic.nearest_ref(x, h, w), want.contiguous()), (H, W, h, w)
        for defect in ("nearest-exact-ratio", "nearest-round"):
            pred = any(bool((ic.nearest_index(i, o, defect) != ic.nearest_index(i, o)).any()) for i, o in ((H, h), (W, w)))
            assert (not oc.same_bits(ic.nearest_ref(x, h, w, defect), want.contiguous())) == pred, (defect, H, W, h, w)
            differ[defect] += pred
    print(f"IMG-NEAREST sweep of {len(ic.NEAREST_SWEEP)} launches: the exact-ratio rule differs on {differ['nearest-exact-ratio']}, "
          f"rounding on {differ['nearest-round']}")
    assert differ["nearest-exact-ratio"] >= 1 and differ["nearest-round"] >= 1


@functools.lru_cache(None)
def _flow_of(cid):
    return _args(ic.BY_ID[cid])["flow"]


def test_flow_reference_is_the_oracle():
    from oracle.output import flow_to_image, make_color_wheel
    assert bool((ic._wheel()[:55] == make_color_wheel()).all())
    for c in BY_OP["flow_to_image"]:
        flow = _flow_of(c.id)
        ref = ic.flow_ref(flow)
        nanpix = torch.isnan(flow).any(-1)
        if c.meta["kind"] != "nan":
            assert not bool(nanpix.any())
            assert bool((torch.from_numpy(flow_to_image(flow)) == ref).all()), c.id
            continue
        # NaN pixels: black; every other pixel as if they held zero flow.  (The oracle itself blackens them too, but its
        # max(-1, nan) negates the rest: not copied, include/mofa_hip.h)
        assert int(nanpix.sum()) == 3
        clean = flow.clone()
        clean[nanpix] = 0
        want = torch.from_numpy(flow_to_image(clean))
        assert bool((ref[~nanpix] == want[~nanpix]).all()) and bool((ref[nanpix] == 0).all()) and bool((want[nanpix] == 255).all()), c.id
        with np.errstate(invalid="ignore"):
            assert bool((torch.from_numpy(flow_to_image(flow))[nanpix] == 0).all())


def test_flow_fragile_byte_conditions():
    """small cases: no byte of the reference moves when the angle moves by -+delta, so the GPU must be bit-equal (the axes family
    is bit-equal by the issue's rule, without this condition); 513 x 512: the reference's own share is at most 5e-5"""
    for c in BY_OP["flow_to_image"]:
        ref, lo, hi = ic.flow_ref(_flow_of(c.id), ranges=True)
        moved = (lo != ref) | (hi != ref)
        assert bool((lo <= ref).all()) and bool((ref <= hi).all())
        if c.big:
            share = float(moved.double().mean())
            print(f"IMG-FRAGILE {c.id}: {share:.2e} of the bytes move under +-delta")
            assert 0 < share <= ic.BIG_OWN_FRAC, (c.id, share)
            want = c.ref({"flow": _flow_of(c.id)})
            assert want.frac == ic.BIG_FRAC == 1e-4 and bool((want.lo == lo).all()) and bool((want.hi == hi).all())
        else:
            want = c.ref({"flow": _flow_of(c.id)})
            assert want.frac == 0.0 and want.lo is want.ref and want.hi is want.ref
            if c.meta["kind"] != "axes":
                assert not bool(moved.any()), (c.id, int(moved.sum()))
    assert ic.DELTA == 2.0 ** -22


# ---- a correct implementation passes, the mutants fail ----------------------------------------------------------------------
@functools.lru_cache(None)
def _truth(cid):
    case = ic.BY_ID[cid]
    r = ic.run_case(ic.impl(None), case, "cpu")
    worst, errs = ic.check_run(case, r)
    return worst, errs, r.placed["out"].t.clone()


@pytest.mark.parametrize("case", ic.CASES, ids=repr)
def test_reference_implementation_passes(case):
    worst, errs, _ = _truth(case.id)
    assert not errs, errs
    assert worst <= 0.5, (case.id, worst)         # the fp64 reference rounded once: u32 |ref|, at most a k-th / a tenth of a bound


def test_checker_sees_a_written_guard_and_an_unwritten_output():
    case = ic.BY_ID["flow_to_image/gauss-7x9-s0"]

    class Stray:
        @staticmethod
        def flow_to_image(flow, out, ws):
            ic.impl(None).flow_to_image(flow, out, ws)
            flow.view(-1)[0] = 1.0                                   # a write to a read-only argument
    r = ic.run_case(Stray, case, "cpu")
    assert any("read-only flow" in e for e in ic.check_run(case, r)[1])

    class Short:
        @staticmethod
        def flow_to_image(flow, out, ws):
            out.view(-1)[:-1] = ic.flow_ref(flow).view(-1)[:-1]      # the last byte stays 0xA5
    r = ic.run_case(Short, case, "cpu")
    assert ic.check_run(case, r)[1]
    r = ic.run_case(ic.impl(None), case, "cpu")
    r.placed["ws"].buf[3] = 0                                        # a byte in front of the workspace
    r.placed["out"].buf[-1] = 0
    errs = ic.check_run(case, r)[1]
    assert any("guard of ws" in e for e in errs) and any("guard of out" in e for e in errs)


@pytest.mark.parametrize("defect", ic.MUTANTS)
def test_mutant_fails_exactly_where_predicted(defect):
    for case in ic.CASES:
        if case.op not in ic.MUTANT_OPS[defect] or (case.big and not defect.startswith("maxrad")):
            continue                                                 # (513 x 512: the checker the small cases of the op prove)
        _, terrs, tout = _truth(case.id)
        assert not terrs, terrs
        r = ic.run_case(ic.impl(defect), case, "cpu")
        _, errs = ic.check_run(case, r)
        if ic.mutant_differs(defect, case):
            assert errs, f"{case.id}: mutant {defect} passes"
            CAUGHT[defect] += 1
        else:
            assert not errs, (case.id, defect, errs)
    print(f"IMG-MUTANT {defect}: caught on {CAUGHT[defect]} cases")
    assert CAUGHT[defect] >= 1, defect
