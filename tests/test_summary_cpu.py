"""The column summary of include/st_abi.h ("column summary") without a GPU: st_summary.h's serial host
form -- the key, limb-add, normalise and rounding functions the kernels call, in a stand-alone
program (tests/native/summary_cpu_check.cpp, also built with AddressSanitizer and
UndefinedBehaviorSanitizer and run directly) -- against the restatement of tests/summary_ref.py on
every table of tests/summary_cases.py, three ways: the defaults, every column down the general path,
and a normalisation every 64 additions.  Fields are compared as bit patterns.  st_summary_text (a
host call of the library) and the program's text are checked against write_csv_ref's number text.
The device must give the same summaries (tests/test_summary_gpu.py)."""
import math

import numpy as np
import pytest

import splat_hip as sh
import summary_cases as sc
import summary_ref as ref

CASES = sorted(sc.tables())


def check(case, got):
    for (name, _), g, w in zip(sc.tables()[case], got, sc.expected(case)):
        print(case, name, g)
        bad = ref.same(g, w)
        assert bad is None, (case, name, bad)


@pytest.mark.parametrize('case', CASES)
def test_serial_form_equals_the_restatement(case, tmp_path):
    cols = sc.tables()[case]
    big = case == 'sum_u32_max'  # two million rows: one sanitized run, one optimised
    got, fast = sc.native(cols, tmp_path, sanitize=True)
    check(case, got)
    assert fast == [ref.fast_path(a) for _, a in cols]
    exact, fast_exact = sc.native(cols, tmp_path, exact=True, sanitize=not big)
    check(case, exact)
    assert not any(fast_exact)
    flushed, _ = sc.native(cols, tmp_path, flush=64, sanitize=not big)
    check(case, flushed)
    # the optimised build gives the same records and takes the same paths
    optimised, fast_optimised = sc.native(cols, tmp_path)
    check(case, optimised)
    assert fast_optimised == fast


def test_which_columns_take_the_fast_path(tmp_path):
    """integers and narrow float spans fit an int128; the full float32 and float64 spans decline"""
    cols = dict(sc.tables()['sum'])
    names = ['f32_cancel', 'f64_tie_even', 'f64_sticky', 'f32_full_span', 'f32_full_span_neg', 'f64_full_span',
             'i32_extremes', 'f64_excursion', 'f64_zeros']
    _, fast = sc.native([(k, cols[k]) for k in names], tmp_path)
    want = dict(f32_cancel=True, f64_tie_even=True, f64_sticky=False, f32_full_span=False, f32_full_span_neg=False,
                f64_full_span=False, i32_extremes=True, f64_excursion=True, f64_zeros=True)
    assert dict(zip(names, fast)) == want
    _, fast = sc.native(sc.tables()['sum_u32_max'], tmp_path)
    assert fast == [True]
    _, fast = sc.native(sc.tables()['len_4097'], tmp_path)
    assert fast[:6] == [True] * 6  # the integer types always fit


def test_expected_values_the_rules_name():
    """the restatement itself on the sums the rules spell out"""
    e = dict(zip([k for k, _ in sc.tables()['sum']], sc.expected('sum')))
    assert e['f32_cancel'].sum == 1.0
    assert e['f64_tie_even'].sum == 2.0 ** 53 and e['f64_tie_up'].sum == 2.0 ** 53 + 4
    assert e['f64_sticky'].sum == 2.0 ** 53 + 2
    assert e['f64_subnormals'].sum == 3 * 2.0 ** -1074
    assert e['f64_overflow'].sum == math.inf and e['f64_overflow_neg'].sum == -math.inf
    assert e['f64_excursion'].sum == 1.7e308
    assert e['f64_just_below_overflow'].sum == np.finfo(np.float64).max and e['f64_just_at_overflow'].sum == math.inf
    assert e['f64_overflow'].ssd == math.inf and e['f64_overflow'].std_dev == math.inf
    u = sc.expected('sum_u32_max')[0]
    assert u.sum == float(0xFFFFFFFF * 2_097_153 + 1) and 0xFFFFFFFF * 2_097_153 > 2 ** 53  # rounds up: not a double
    z2, z3 = (dict(zip([k for k, _ in sc.tables()['median']], sc.expected('median')))[k] for k in ('zeros_2', 'zeros_3'))
    assert ref.bits(z2.min) == 1 << 63 and ref.bits(z2.max) == 0 and ref.bits(z2.median) == 0
    assert ref.bits(z3.median) == 1 << 63
    d = dict(zip([k for k, _ in sc.tables()['deviation']], sc.expected('deviation')))
    assert d['t_overflow'].ssd == math.inf and d['sum_inf'].std_dev == math.inf
    assert d['d124_float64'].mean == 7 / 3


@pytest.mark.parametrize('case', ['sum', 'median', 'deviation', 'same_name', 'len_0'])
def test_text(case, tmp_path):
    names = [k for k, _ in sc.tables()[case]]
    want = ref.text(names, sc.expected(case))
    assert sc.native_text(names, sc.expected(case), tmp_path, sanitize=True) == want
    got = sh.summary_text([(k, None) for k in names], [sh.ColSummary(*s) for s in sc.expected(case)])
    assert got == want
    assert want.startswith(b'column,rows,nanCount,infCount,min,max,mean,stdDev,median\n') and want.endswith(b'\n')
    assert want.count(b'\n') == 1 + len(names)


def test_text_spells_the_special_values(tmp_path):
    s = ref.Summary(3, 1, 2, -0.0, math.inf, 0.0, math.nan, 0.0, -math.inf, 1e21)
    got = sh.summary_text([('a,b', None)], [sh.ColSummary(*s)])
    assert got == b'column,rows,nanCount,infCount,min,max,mean,stdDev,median\na,b,3,1,2,0,Infinity,NaN,-Infinity,1e+21\n'
    with pytest.raises(sh.StError) as e:
        sh.summary_text([], [])
    assert e.value.code == sh.ST_ERR_ARG
