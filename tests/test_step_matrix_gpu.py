"""Every case of tests/step_cases.py through ``mofa_video_amd.ops`` on the GPU: the layout movers ``nchw_to_tokens`` /
``tokens_to_nchw`` (every channel-tile class against every pixel-tile class, the four output forms, the rounding family) and the
scheduler step kernels ``prepare_model_input(_dev)`` / ``cfg_euler_step(_dev)_`` (T x HW, four rows of the step table, the exact
cases, one second-pass case per kernel).

Per case: guards intact (compared as bits), read-only arguments bit-unchanged, and the comparison the table states -- exact bits,
or |out - fp64 reference| <= the derived bound per element (step_cases docstring; tests/test_step_cases_cpu.py proves the
references, the exact families and that each check fails on a wrong kernel).  Each comparison prints its worst err / bound
(pytest -s), ``test_worst_ratio_per_op`` the worst per op.  ``test_scalar_forms_agree`` runs the host-scalar and the
device-scalar form of every step on the same data: latents bit-equal, model input within one fp16 ulp.

``test_argument_edges_rejected_without_launch`` goes through the C ABI: every call returns MOFA_EINVAL and leaves its NaN-filled
buffers bit-unchanged."""
import collections

import pytest
import torch

import aux_cases as ac
import op_cases as oc
import step_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = collections.defaultdict(float)


@pytest.fixture(scope="module")
def ops():
    from mofa_video_amd import lib
    from mofa_video_amd import ops as o
    lib.load()
    return o


@pytest.mark.parametrize("case", sc.CASES, ids=repr)
def test_hip_op_meets_its_reference(ops, case):
    r = oc.run(ops, case, DEV)
    worst, errs = sc.check_run(case, r)
    off = "; ".join(f"{k.split()[-1]} {n} / {m} elements off the reference rounded once" for k, (n, m) in ac.OFF_ROUNDING.items()
                    if k.startswith(case.id + " "))
    print(f"STEP {case.id}: worst err / bound {worst:.3f} ({off})" if worst else f"STEP {case.id}: bit-equal / exact")
    WORST[case.op] = max(WORST[case.op], worst)
    assert not errs, errs
    if case.op == "nchw_to_tokens" and case.meta["family"] == "P":   # out= forms against the fresh output (family R holds
        oc.check_out_is_honoured(ops, case, DEV, r)                   # the infinities and a NaN on purpose)
    if case.op == "tokens_to_nchw":
        assert torch.isfinite(r.ret).all(), f"{case.id}: a NaN column of the input rows reached the result"


@pytest.mark.parametrize("pair", sc.pairs(), ids=lambda p: p[0].id)
def test_scalar_forms_agree(ops, pair):
    host, dev = pair
    a, b = oc.run(ops, host, DEV).outputs()[0][1], oc.run(ops, dev, DEV).outputs()[0][1]
    if host.op in sc._EULER:
        assert oc.same_bits(a, b), f"{host.id}: device-scalar and host-scalar Euler steps differ"
    else:
        ulps = (oc.bits(a[:, :4]).int() - oc.bits(b[:, :4]).int()).abs().max().item()
        print(f"STEP {host.id}: model input, device-scalar vs host-scalar form: {ulps} fp16 ulp")
        assert ulps <= 1 and oc.same_bits(a[:, 4:8], b[:, 4:8]), (host.id, ulps)


def test_worst_ratio_per_op():
    for op in sc.OPS:
        print(f"STEP-WORST {op}: {WORST[op]:.3f}")


def test_argument_edges_rejected_without_launch(ops):
    from mofa_video_amd import lib as L
    lib = L.load()
    st = L.stream_ptr()
    EINVAL = -22
    # sized for the largest output either reading of any argument list below could produce (65536 images of one channel and one
    # pixel; 4 frames of 64 pixels at ld 24): nothing here can write out of bounds even where a check is missing
    h1 = torch.full((4096, 64), ac.NAN, dtype=oc.F16, device=DEV)
    h2 = torch.full((4096, 64), ac.NAN, dtype=oc.F16, device=DEV)
    f1 = torch.full((65536,), ac.NAN, dtype=oc.F32, device=DEV)
    f2 = torch.full((65536,), ac.NAN, dtype=oc.F32, device=DEV)
    tab = torch.full((64,), ac.NAN, dtype=oc.F32, device=DEV)
    cnt = torch.zeros(4, dtype=torch.int32, device=DEV)
    bufs = (h1, h2, f1, f2, tab, cnt)
    snaps = [b.clone() for b in bufs]
    H1, H2, F1, F2, TAB, CNT = (L.ptr(b) for b in bufs)

    def n2t(x=F1, y=H1, n=2, C=4, HW=8, ldo=8):
        return lib.mofa_nchw_f32_to_nhwc_f16(x, y, n, C, HW, ldo, 1.0, st)

    def t2n(x=H1, y=F1, n=2, C=4, HW=8, ldx=8):
        return lib.mofa_nhwc_f16_to_nchw_f32(x, y, n, C, HW, ldx, st)

    def prep(lat=F1, img=F2, out=H1, T=4, HW=64, ldo=24, sigma=1.5):
        return lib.mofa_prepare_model_input(lat, img, out, T, HW, ldo, sigma, st)

    def prep_dev(lat=F1, img=F2, out=H1, T=4, HW=64, ldo=24, scal=TAB):
        return lib.mofa_prepare_model_input_dev(lat, img, out, T, HW, ldo, scal, st)

    def euler(lat=F1, np_=H1, T=4, HW=64, ldn=16, sigma=1.5, sigma_next=1.0):
        return lib.mofa_cfg_euler_step(lat, np_, T, HW, ldn, sigma, sigma_next, 1.0, 3.0, st)

    def euler_dev(lat=F1, np_=H1, T=4, HW=64, ldn=16, scal=TAB):
        return lib.mofa_cfg_euler_step_dev(lat, np_, T, HW, ldn, scal, 1.0, 3.0, st)
    calls = {}
    for name, fn in (("nchw_to_tokens", n2t), ("tokens_to_nchw", t2n)):
        ld = "ldo" if fn is n2t else "ldx"
        calls.update({f"{name} NULL x": lambda fn=fn: fn(x=None), f"{name} NULL y": lambda fn=fn: fn(y=None),
                      f"{name} n 0": lambda fn=fn: fn(n=0), f"{name} n -1": lambda fn=fn: fn(n=-1), f"{name} C 0": lambda fn=fn: fn(C=0),
                      f"{name} HW 0": lambda fn=fn: fn(HW=0), f"{name} HW -8": lambda fn=fn: fn(HW=-8),
                      f"{name} ld < C": lambda fn=fn, ld=ld: fn(**{ld: 3}),
                      f"{name} n 65536": lambda fn=fn, ld=ld: fn(n=65536, C=1, HW=1, **{ld: 1})})
    for name, fn in (("prepare_model_input", prep), ("prepare_model_input_dev", prep_dev)):
        calls.update({f"{name} NULL latents": lambda fn=fn: fn(lat=None), f"{name} NULL image": lambda fn=fn: fn(img=None),
                      f"{name} NULL out": lambda fn=fn: fn(out=None), f"{name} T 0": lambda fn=fn: fn(T=0),
                      f"{name} HW 0": lambda fn=fn: fn(HW=0), f"{name} T -1": lambda fn=fn: fn(T=-1),
                      f"{name} ldo % 8": lambda fn=fn: fn(ldo=20), f"{name} ldo < 8": lambda fn=fn: fn(ldo=0),
                      f"{name} ldo -8": lambda fn=fn: fn(ldo=-8)})
    calls["prepare_model_input_dev NULL scalars"] = lambda: prep_dev(scal=None)
    for name, fn in (("cfg_euler_step", euler), ("cfg_euler_step_dev", euler_dev)):
        calls.update({f"{name} NULL latents": lambda fn=fn: fn(lat=None), f"{name} NULL prediction": lambda fn=fn: fn(np_=None),
                      f"{name} T 0": lambda fn=fn: fn(T=0), f"{name} HW 0": lambda fn=fn: fn(HW=0), f"{name} HW -1": lambda fn=fn: fn(HW=-1),
                      f"{name} ldn % 4": lambda fn=fn: fn(ldn=6)})
    calls.update({"cfg_euler_step sigma 0": lambda: euler(sigma=0.0), "cfg_euler_step sigma < 0": lambda: euler(sigma=-1.5),
                  "cfg_euler_step_dev NULL scalars": lambda: euler_dev(scal=None),
                  "step_select nsteps 0": lambda: lib.mofa_step_select(TAB, CNT, F2, 0, st),
                  "step_select nsteps -1": lambda: lib.mofa_step_select(TAB, CNT, F2, -1, st),
                  "step_select NULL table": lambda: lib.mofa_step_select(None, CNT, F2, 8, st),
                  "step_select NULL counter": lambda: lib.mofa_step_select(TAB, None, F2, 8, st),
                  "step_select NULL cur": lambda: lib.mofa_step_select(TAB, CNT, None, 8, st)})
    wrong = {name: rc for name, rc in ((name, call()) for name, call in calls.items()) if rc != EINVAL}
    torch.cuda.synchronize()
    assert not wrong, f"accepted (return code): {wrong}"
    for b, s in zip(bufs, snaps):
        assert oc.same_bits(b, s), "a rejected call wrote to a buffer"
