"""The warp's case table (tests/splat_cases.py) on the CPU, no device: the fp64 reference rounded once passes every case through
the very checks the GPU run gets (tests/test_splat_matrix_gpu.py); every "wrong kernel" mutant fails the cases its map names; the
constructions deliver the segment lengths and tiny normalisers they promise; the exact families leave out at most 1 % of their
elements; the summation-order check is not vacuous; the reference agrees with ``oracle.softsplat`` on the Gaussian cases; and the
argument rules of ``mofa_softsplat_avg_f16`` (include/mofa_hip.h) hold before any device call."""
import os
import subprocess

import pytest
import torch

import splat_cases as sc
from test_softsplat_grad_cpu import A, ROOT


@pytest.mark.parametrize("case", sc.CASES, ids=repr)
def test_reference_passes_and_constructions_hold(case):
    good = sc.standin()
    worst, errs = sc.check_run(case, sc.Run(case, good), good)
    assert not errs, errs
    assert worst <= 1.0
    wants = case.want()
    for (i, t), k in case.counts.items():
        assert int(wants[i].n[t]) == k, (case.id, i, t, int(wants[i].n[t]), k)
    if case.exact:                                                    # the share the exact check leaves out, on the reference alone
        left, total = sc.LEFT_OUT[case.id]
        assert total > 0 and left <= 0.01 * total, (case.id, left, total)
        assert max(int(w.n.max()) for w in wants) <= sc.N_EXACT


def test_table_covers_what_it_claims():
    ids = set(sc.BY_ID)
    for H, W in sc.PLANES:
        for C in (sc.WIDTHS if (H, W) in sc.FULL else (8, 520)):
            assert f"dyadic/{H}x{W}-C{C}" in ids and any(i.startswith(f"gauss/{H}x{W}-C{C}-mag1.5") for i in ids), (H, W, C)
        assert f"gauss/{H}x{W}-C8-mag4-n1" in ids
    assert sorted({H * W % 4 for H, W in sc.PLANES}) == [0, 1, 2, 3]
    assert {1023, 1024, 1025} <= {H * W for H, W in sc.PLANES} and any(-(-H * W // sc.SCAN_THREADS) == 3 for H, W in sc.PLANES)
    for H, W in sc.FULL:
        assert sc.BY_ID[f"gauss/{H}x{W}-C8-mag1.5-n3"].singles
    # segment lengths on both sides of the insertion / heap switch, and the tiny normalisers as stated
    seg = sorted(set(sc.BY_ID["segments/12x20"].counts.values()))
    assert seg == [1, sc.SS_INSERTION_MAX - 1, sc.SS_INSERTION_MAX, sc.SS_INSERTION_MAX + 1, 200]
    tiny = sc.BY_ID["tiny/7x9"]
    e = sc.entries(tiny.inputs()[1][0], 7, 9)
    assert sorted(e.w64.tolist()) == [2.0 ** -30, 2.0 ** -24, 2.0 ** -20] and sorted(e.tgt.tolist()) == sorted(t for _, t in sc.TINY)
    # the special source contributes nowhere and its own pixel keeps zero-weight entries only
    sp = sc.BY_ID["special/7x9"]
    t = sc.SPECIAL_AT[0] * 9 + sc.SPECIAL_AT[1]
    for i, w in enumerate(sp.want()):
        assert bool(w.zero[t]) and int(w.n[t]) == 3 and int(w.zero.sum()) == 1, i
        assert not bool((sc.entries(sp.inputs()[1][i], 7, 9).src == t).any()), i


@pytest.mark.parametrize("defect", sc.MUTANTS)
def test_every_mutant_fails_its_cases(defect):
    bad = sc.standin(defect)
    for cid in sc.MUTANT_CASES[defect]:
        case = sc.BY_ID[cid]
        _, errs = sc.check_run(case, sc.Run(case, bad), bad)
        assert errs, f"the wrong kernel {defect} passes {cid}"


def test_column_subset_check_on_the_standin():
    assert not sc.column_subset_errors(sc.standin())

    def leaky(feat, flow, out, H, W):                                 # a warp whose first channel depends on the width
        sc.standin()(feat, flow, out, H, W)
        if feat.shape[1] > 8:
            out[:, 0] = out[:, 0] * 2
        return []
    assert sc.column_subset_errors(leaky)


def test_summation_order_check_is_not_vacuous():
    """on the inputs of the order check the source-major sum differs from the key-order sum in at least one bit"""
    from op_cases import same_bits
    for cid in sc.ORDER_CASES:
        case = sc.BY_ID[cid]
        flow = case.inputs()[1]
        key = sc.norm_emulation(flow, case.H, case.W)
        assert same_bits(key, sc.norm_emulation(flow, case.H, case.W)), cid
        nw = torch.stack([sc.splat_sums(case.inputs()[0].double(), sc.entries(flow[i], case.H, case.W))[2]
                          for i in range(flow.shape[0])]).reshape(key.shape)
        assert bool(((key.double() - nw).abs() <= 200 * sc.U32 * nw).all()), cid      # n u32 Nw, n <= 240 less the exact first sum
    case = sc.BY_ID["segments/12x20"]
    flow = case.inputs()[1]
    assert not same_bits(sc.norm_emulation(flow, case.H, case.W), sc.norm_emulation(flow, case.H, case.W, order="source"))


GAUSS = [c for c in sc.CASES if c.cls == "gauss" and c.C <= 520]


@pytest.mark.parametrize("case", GAUSS, ids=repr)
def test_reference_agrees_with_the_oracle(case):
    """``oracle.softsplat`` is the same sum in fp32 (rounded products, rounded sums, a correctly rounded division): it lies within
    the fp32 part of the bound of the fp64 reference"""
    from oracle.softsplat import softsplat
    feat, flow = case.inputs()
    H, W, C = case.H, case.W, case.C
    img = feat.float().reshape(1, H, W, C).permute(0, 3, 1, 2).contiguous()
    for i, w in enumerate(case.want()):
        got = softsplat(img, flow[i:i + 1], None, "avg")[0].permute(1, 2, 0).reshape(H * W, C).double()
        fp32_part = w.bound - sc.U16 * w.ref.abs() - 2.0 ** -25
        assert bool(((got - w.ref).abs() <= fp32_part + 2.0 ** -150).all()), (case.id, i, ((got - w.ref).abs() - fp32_part).max().item())


# ---- argument rules (include/mofa_hip.h), no device -----------------------------------------------------------------------------
def _avg(l, feat=A, flow=A, out=A, ws=A, nflows=1, H=4, W=4, C=8, ldf=8, ldo=8):
    return l.mofa_softsplat_avg_f16(feat, flow, out, ws, nflows, H, W, C, ldf, ldo, None)


def test_bad_arguments_are_refused_without_gpu():
    from mofa_video_amd import lib
    l = lib.load()
    bad = [dict(feat=None), dict(flow=None), dict(out=None), dict(ws=None),
           dict(C=0), dict(C=-8), dict(C=4), dict(C=12), dict(ldf=12), dict(ldf=4), dict(ldo=12), dict(ldo=-4),
           dict(nflows=0), dict(nflows=-1), dict(nflows=65536),
           dict(H=0), dict(H=-4), dict(W=0), dict(W=-1),
           dict(H=1 << 15, W=1 << 14), dict(H=1, W=1 << 29), dict(H=1 << 29, W=1),      # H * W = 2^29
           dict(H=65536, W=65536)]                                                      # H * W = 2^32: 0 as an int
    for b in bad:
        assert _avg(l, **b) == -22, b


def test_workspace_size_is_formed_in_64_bits():
    from mofa_video_amd import lib
    l = lib.load()
    for n, H, W in ((1, 7, 9), (24, 72, 128), (65535, 1, (1 << 29) - 1), (3, 1 << 16, 1 << 13), (1, 65536, 65536), (2, 46341, 46341)):
        assert l.mofa_softsplat_ws_bytes(n, H, W) == (11 * H * W + 1) * 4 * n + 64, (n, H, W)


HOST_MAIN = r"""
#include "%s"
#include <cstdio>
#include <cstdlib>
// prints ss_avg_check for every (nflows H W C ldf ldo) on the command line: the host arithmetic alone, nothing is launched
int main(int argc, char** argv) {
    const void* a = (const void*)0x10000;
    for (int i = 1; i + 5 < argc; i += 6) {
        int v[6];
        for (int j = 0; j < 6; ++j) v[j] = (int)strtol(argv[i + j], nullptr, 10);
        printf("%%d\n", ss_avg_check(a, (const float*)a, a, a, v[0], v[1], v[2], v[3], v[4], v[5]));
    }
    return 0;
}
"""


def test_last_accepted_values_pass_the_host_check(tmp_path):
    """the limits are not off by one: the host-side check of mofa_softsplat_avg_f16, compiled into a stand-alone program that calls
    nothing else, accepts the last value of every limit (no launch: these shapes are never run) and refuses the next one"""
    from mofa_video_amd import _build
    src, exe = str(tmp_path / "ss_avg_check_main.hip"), str(tmp_path / "ss_avg_check_main")
    with open(src, "w") as f:
        f.write(HOST_MAIN % os.path.join(ROOT, "mofa_video_amd", "csrc", "softsplat.hip"))
    subprocess.run([_build._hipcc(), "--offload-arch=gfx950", "-O1", "-std=c++17", src, "-o", exe], check=True)
    P = (1 << 29) - 1
    rows = [((65535, 4, 4, 8, 8, 8), 0), ((65536, 4, 4, 8, 8, 8), -22), ((1, 1, P, 8, 8, 8), 0), ((1, P, 1, 8, 8, 8), 0),
            ((1, 1, P + 1, 8, 8, 8), -22), ((65535, 1, P, 8, 8, 8), 0), ((1, 23170, 23170, 8, 8, 8), 0), ((1, 23171, 23171, 8, 8, 8), -22),
            ((1, 65536, 65536, 8, 8, 8), -22), ((1, 1, 1, 8, 8, 8), 0), ((1, 1, 1, 2147483640, 2147483640, 2147483640), 0),
            ((1, 4, 4, 7, 8, 8), -22)]
    out = subprocess.run([exe] + [str(v) for r, _ in rows for v in r], check=True, capture_output=True, text=True).stdout.split()
    assert [int(o) for o in out] == [rc for _, rc in rows], list(zip(rows, out))
