"""The scalar rules of splat-transform_amd/csrc/st_jsmath.h compiled for the host
(tests/native/jsmath_cpu_check.cpp, built with the library's flags and again under AddressSanitizer
and UndefinedBehaviorSanitizer): V8's own values of tests/golden/mathfns bit for bit, fdlibm's stated
error bound against mpmath on tests/probe_cases.py's wider set, and the exact operations against
exact references.  tests/test_probe_scalar_gpu.py holds the device compile to the same program."""
import numpy as np
import pytest

import probe_cases as pc
from golden_io import Golden

BUILDS = [pytest.param(False, id='plain'), pytest.param(True, id='asan_ubsan')]
# fixture array -> (op, its scalar)
MATHFNS = {'exp': ('exp', 0.0), 'log': ('log', 0.0), 'log1abs': ('log1abs', 0.0), 'sigmoid': ('sigmoid', 0.0),
           'logtransform': ('log_transform', 0.0), 'logexp_s05': ('logexp', 0.5), 'logexp_s2': ('logexp', 2.0)}


def same(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f'{what}: {len(bad)} differ, first at {bad[:5]}: {got[bad[:5]]} != {want[bad[:5]]}'


@pytest.mark.parametrize('sanitize', BUILDS)
@pytest.mark.parametrize('name', sorted(MATHFNS))
def test_header_gives_v8s_values_bit_for_bit(name, sanitize):
    g = Golden('mathfns')
    op, s = MATHFNS[name]
    same(pc.host(op, g['x'], s=s, sanitize=sanitize), pc.bits(g[name]), name)


@pytest.mark.parametrize('op', pc.ONE_INPUT + pc.TWO_INPUT)
def test_sanitized_build_gives_the_plain_builds_bits(op):
    """every op over the wider set under ASan + UBSan: no report, and the -O3 build's results"""
    two = op in pc.TWO_INPUT
    a, b = pc.pair_inputs() if two else (pc.wide_inputs(), None)
    same(pc.host(op, a, b, s=pc.LOGEXP_S, sanitize=True), pc.host_wide(op), op)


def test_wide_set_is_what_it_says():
    x = pc.wide_inputs()
    assert 38_000 <= len(x) <= 50_000
    b = set(int(v) for v in pc.bits(x))
    for h in pc.EXP_HI_WORDS[:4]:
        for sign in (0, pc.SIGN):
            assert all(v in b for v in pc._around(sign | (h << 32)))
    # the k edges really are edges
    for kk in (-1022, -1021, 1023, 1024):
        e = pc.exp_k_edge(kk)
        assert pc.exp_k(float(pc.f64([e])[0])) == kk and pc.exp_k(float(pc.f64([e - 1])[0])) == kk - (1 if kk > 0 else -1)
        assert e in b and e - 2 in b and e + 2 in b
    with np.errstate(over='ignore'):
        ex = np.exp(x[np.isfinite(x)])
    assert ((ex > 0) & (ex < 2.0 ** -1022)).sum() >= 1000  # inputs whose exp is subnormal
    assert ((x != 0) & (np.abs(x) < 2.0 ** -1022)).sum() >= 1000  # subnormal inputs


# fdlibm's stated bound: the error of exp and log is below 1 ulp.  For a subnormal result exp's
# last multiply (y * twopk * twom1000) rounds once more, onto the subnormals' grid: at most half a
# grid step on top, 1.5 steps in all.
@pytest.mark.parametrize('op', ['exp', 'log'])
def test_exp_log_within_fdlibms_bound_of_mpmath(op):
    import mpmath
    x = pc.wide_inputs()
    got = pc.f64(pc.host_wide(op))
    want_finite = np.isfinite(x) & (x > 0 if op == 'log' else np.ones(len(x), bool))
    fin = want_finite & np.isfinite(got)
    if op == 'exp':
        # the values that overflowed: exactly the x above ln(2^1024 - 2^970), where rounding gives Infinity
        with mpmath.workprec(200):
            limit = mpmath.log(mpmath.mpf(2) ** 1024 - mpmath.mpf(2) ** 970)
            over = np.array([mpmath.mpf(float(v)) >= limit for v in x[want_finite]])
        assert np.array_equal(np.isinf(got[want_finite]), over)
    else:
        assert fin.sum() == want_finite.sum()
    err, sub = pc.ulp_errors(mpmath.exp if op == 'exp' else mpmath.log, x[fin], got[fin])
    print(f'{op}: max error {err[~sub].max():.4f} ulp over {(~sub).sum()} normal results' +
          (f', {err[sub].max():.4f} grid steps over {sub.sum()} subnormal results' if sub.any() else ''))
    assert err[~sub].max() < 1.0
    if sub.any():
        assert err[sub].max() <= 1.5


def test_exp_log_special_values():
    x = pc.wide_inputs()
    b = pc.bits(x)
    e, lg = pc.host_wide('exp'), pc.host_wide('log')
    nan = np.isnan(x)
    # a NaN argument comes back as x + x: quiet, sign and payload kept
    same(e[nan], b[nan] | np.uint64(1 << 51), 'exp of NaN')
    neg = (b >> np.uint64(63)) == 1
    same(lg[nan & ~neg], b[nan & ~neg] | np.uint64(1 << 51), 'log of a positive NaN')
    # V8's log of anything with the sign bit set except -0: the signalling NaN
    same(lg[neg & (x != 0)], np.full((neg & (x != 0)).sum(), 0x7ff4000000000000, np.uint64), 'log of a negative')
    same(lg[x == 0], np.full((x == 0).sum(), pc._b(-np.inf), np.uint64), 'log of a zero')
    same(e[x == -np.inf], np.zeros((x == -np.inf).sum(), np.uint64), 'exp(-Infinity)')
    assert e[b == pc._b(1.0)][0] == pc._b(np.e) and e[b == 0][0] == pc._b(1.0) and lg[b == pc._b(1.0)][0] == 0


def test_exact_ops_against_exact_references():
    x = pc.wide_inputs()
    with np.errstate(all='ignore'):
        for op, want in (('sqrt', np.sqrt(x)), ('round', np.floor(x + 0.5))):
            got = pc.host_wide(op)
            ok = ~np.isnan(want)
            same(got[ok], pc.bits(want)[ok], op)
            assert np.isnan(pc.f64(got)[~ok]).all()
        # a NaN that sqrt makes is x86's default NaN; a NaN argument is quieted
        made = (x < 0) & ~np.isnan(x)
        assert (pc.host_wide('sqrt')[made] == pc.X86_NAN).all()
        same(pc.host_wide('sqrt')[np.isnan(x)], pc.bits(x)[np.isnan(x)] | np.uint64(1 << 51), 'sqrt of NaN')
        cast = pc.host_wide('f32_cast')
        ok = ~np.isnan(x)
        same(cast[ok], x.astype(np.float32).view(np.uint32)[ok], 'f32_cast')
    same(pc.host_wide('f32_store'), pc.ref_f32_store(x), 'f32_store')
    same(cast[~ok], pc.ref_f32_store(x)[~ok], 'f32_cast of NaN')  # cvtsd2ss's own rule is f32_store's
    same(pc.host_wide('to_int32'), pc.ref_to_int32(x), 'to_int32')
    same(pc.host_wide('to_uint8'), pc.ref_to_uint8(x), 'to_uint8')
    same(pc.host_wide('sign'), pc.ref_sign(x), 'sign_')


def test_named_edge_values():
    def one(op, pattern):
        return int(pc.host(op, pc.f64([pattern]))[0])
    assert one('f32_store', 0x7ff4000000000000) == 0x7fe00000  # js::log's signalling NaN
    assert one('f32_store', pc.X86_NAN) == 0xffc00000
    assert one('f32_store', 0x47EFFFFFF0000000) == 0x7f800000  # the tie above the largest float32 overflows
    assert one('f32_store', 0x47EFFFFFF0000000 - 1) == 0x7f7fffff
    assert one('f32_store', pc._b(2.0 ** -150)) == 0 and one('f32_store', pc._b(2.0 ** -150) + 1) == 1
    assert one('f32_store', pc._b(1.0 + 2.0 ** -24)) == 0x3f800000  # ties go to even, both ways
    assert one('f32_store', pc._b(1.0 + 3 * 2.0 ** -24)) == 0x3f800002
    for v, want in ((2.0 ** 31, -2 ** 31), (-2.0 ** 31, -2 ** 31), (2.0 ** 32 + 1, 1), (2.0 ** 32 - 1, -1), (2.0 ** 53, 0),
                    (2.0 ** 63, 0), (2.0 ** 64, 0), (1e300, 0), (-0.5, 0), (5e-324, 0), (2.0 ** 63 + 2048, 2048),
                    (-(2.0 ** 64 + 4096), -4096), (2.0 ** 83 + 2.0 ** 31, -2 ** 31), (-1.5, -1)):
        assert one('to_int32', pc._b(v)) == want, v
    assert one('sqrt', pc._b(2.0)) == 0x3FF6A09E667F3BCD
    # the quaternion packers' norm, sqrt(2.0) * 0.5, by the program's sqrt and division
    assert int(pc.host('div', pc.f64([0x3FF6A09E667F3BCD]), np.array([2.0]))[0]) == pc._b(0.7071067811865476)
    assert one('round', pc._b(0.49999999999999994)) == pc._b(1.0)  # t + 0.5 rounds up to 1 first
    assert one('round', pc._b(-0.5)) == 0 and one('round', pc._b(-0.75)) == pc._b(-1.0)


def test_two_input_ops():
    a, b = pc.pair_inputs()
    with np.errstate(all='ignore'):
        want = a / b
    got = pc.host_wide('div')
    ok = ~np.isnan(want)
    same(got[ok], pc.bits(want)[ok], 'div')
    nan_in = np.isnan(a) | np.isnan(b)
    assert (got[~ok & ~nan_in] == pc.X86_NAN).all()  # 0 / 0 and Inf / Inf: the machine's default NaN
    one = ~ok & nan_in  # the NaN operand comes back quieted (where both are NaN they are the same one)
    same(got[one], np.where(np.isnan(a), pc.bits(a), pc.bits(b))[one] | np.uint64(1 << 51), 'div of a NaN')
    sub = ok & (want != 0) & (np.abs(want) < 2.0 ** -1022)
    assert sub.sum() >= 1000 and (np.abs(a) < 2.0 ** -1022).sum() >= 1000  # subnormal results and operands
    same(pc.host_wide('min'), pc.ref_minmax(a, b, False), 'min_')
    same(pc.host_wide('max'), pc.ref_minmax(a, b, True), 'max_')
