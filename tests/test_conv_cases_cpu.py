"""The convolution-geometry tables of tests/conv_cases.py proven on the CPU before a GPU sees them: the tables hold the classes
they are there for, the exactness bound of family E holds per case, every case passes its checks through the fp32 stand-in
``emu_ops.igemm`` (F.conv2d; family E by EQUALITY with the per-tap fp64 reference, family A inside the GEMM class, guards
intact), and every "wrong convolution" mutant FAILS family E on every case where it changes the arithmetic -- a checker that
cannot fail proves nothing.  tests/test_igemm_conv_edges_gpu.py runs the same cases through the HIP kernels on every tile.

The mutants (conv_cases.MUTANTS; conv_cases.mutant_differs states from the geometry alone where each changes the arithmetic):
  origin        tap origin off by one                                   every convolution row
  no-dil        dilation ignored                                        rows with dil > 1
  swap-kykx     ky / kx exchanged                                       k > 1 and some off-centre tap meets the image
  col-overrun   a column overrun reads the next row's first pixel       the last tap passes the last column and the flat index stays
                instead of zero                                         inside the buffer (not k3-W1024: one single row)
  up-round-up   up = 2 source pixel rounded up instead of down          rows with up = 2
  clip-late     the clip boundary of convT3 one frame late              convT3 rows with T > 0 (all have two clips or more)
  drop-ktile    one K tile of the tap at offset 0 never arrives          every row of the three tables"""
import pytest
import torch

import conv_cases as cc
import emu_ops


@pytest.fixture(scope="module", autouse=True)
def _release_case_data():
    yield
    cc.release()


def _checked(module, case):
    r = cc.run(module, case, "cpu")
    worst, errs = cc.check_run(case, r)
    return worst, errs, r.placed["out"].t


def _stand_in(s, epis=cc.EPIS):
    """family E through the stand-in by equality for every epilogue, family A for one; -> worst err / bound of family A"""
    d = cc._data(s, "E")
    assert d.units == s.taps * s.Cin * 6 + 128 < cc.E_UNITS_MAX and (d.acc * 16).abs().max().item() <= d.units - 128, s.id
    for epi in epis:
        _, errs, _ = _checked(emu_ops, cc.case(s, "E", epi))
        assert not errs, errs
    worst, errs, _ = _checked(emu_ops, cc.case(s, "A", epis[len(s.id) % len(epis)]))
    assert not errs, errs
    return worst


def test_tables_hold_their_classes():
    cc.assert_table()


@pytest.mark.parametrize("s", cc.CONV_ROWS + cc.SPLIT_ROWS + cc.PIPE_OVER_ROWS, ids=repr)
def test_conv_stand_in(s):
    print(f"CONV-CPU {s.id}: M {s.M}, family A worst err / bound {_stand_in(s):.3f}")


@pytest.mark.parametrize("s", cc.CONVT_ROWS, ids=repr)
def test_convt3_stand_in(s):
    print(f"CONV-CPU {s.id}: M {s.M}, family A worst err / bound {_stand_in(s):.3f}")


@pytest.mark.parametrize("K", cc.PLAIN_K)
def test_plain_stand_in(K):
    top = max(_stand_in(s, (cc.plain_epi(s),)) for s in cc.plain_rows(K))
    print(f"CONV-CPU plain K{K}: {len(cc.plain_rows(K))} cases, family A worst err / bound {top:.3f}")


# ---- mutants ---------------------------------------------------------------------------------------------------------------
def _assert_mutants(s, epis):
    truth = cc.wrong_igemm(s, None)
    d = cc._data(s, "E")
    for epi in epis:
        case = cc.case(s, "E", epi)
        _, terrs, tout = _checked(truth, case)
        assert not terrs, ("the plain fp64 convolution must pass", terrs)
        for defect in cc.MUTANTS:
            differs = cc.mutant_differs(defect, s)
            if epi == epis[0]:                            # the stated rule against the two fp64 accumulators
                rows = int((cc.acc64(s, d.x, d.w, defect) != d.acc).any(1).sum())
                assert (rows > 0) == differs, (s.id, defect, rows)
                if differs:
                    print(f"CONV-MUTANT {s.id} {defect}: {rows} / {s.M} rows differ")
            _, errs, out = _checked(cc.wrong_igemm(s, defect), case)
            if differs:
                assert errs, f"{case.id}: mutant {defect} passes family E"
            else:                                         # no defect on this geometry: asserted equal, not skipped
                assert not errs and cc.oc.same_bits(out, tout), (case.id, defect)


@pytest.mark.parametrize("s", cc.CONV_ROWS, ids=repr)
def test_conv_mutants_fail(s):
    _assert_mutants(s, cc.EPIS)


@pytest.mark.parametrize("s", cc.CONVT_ROWS, ids=repr)
def test_convt3_mutants_fail(s):
    _assert_mutants(s, cc.EPIS)


def test_plain_mutants_fail():
    for s in (cc.plain(64, 257, 72), cc.plain(192, 513, 328), cc.plain(128, 1, 8)):
        _assert_mutants(s, (cc.plain_epi(s),))


def test_every_mutant_fails_somewhere():
    rows = cc.CONV_ROWS + cc.CONVT_ROWS
    for defect in cc.MUTANTS:
        assert sum(cc.mutant_differs(defect, s) for s in rows) >= 3, defect


def test_truth_is_not_a_mutant():
    """the per-tap fp64 sum the mutants are made from agrees with the F.conv2d stand-in on Gaussian data inside fp16 rounding"""
    for s in (cc.CONV_BY_ID["k5d2"], cc.CONV_BY_ID["k3up2-trail-s2"], cc.CONVT_ROWS[4]):
        case = cc.case(s, "A", "r1")
        _, _, a = _checked(cc.wrong_igemm(s, None), case)
        _, _, b = _checked(emu_ops, case)
        assert (a.float() - b.float()).abs().max().item() <= 2.0 ** -9 * a.float().abs().max().item(), s.id
