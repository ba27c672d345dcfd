"""The device-wide primitives of splat-transform_amd/csrc/st_prims.hip called directly through the
test hook st_dev_probe (include/st_abi.h): scan_u32 against numpy's cumsum modulo 2^32, the five
radix-sort entry points against numpy's stable argsort of the sorted bit field, minmax_keys_dev
against the key map in numpy, and iota_u32; at the sizes where the code changes path (one block /
two levels / three levels of the scan; k_sort256 / k_small_sort / the tiled passes of the sorts;
the 512-workgroup cap of min/max), with every output between sentinel words.

The sorts' full product of sizes, bit ranges and key patterns runs up to n = 8,193.  At n = 70,001
and n = 1,048,583 the bit ranges are one per pass count: (3, 11) one pass, (0, 9) two, (0, 17)
three, (7, 32) four (a last digit of one bit, begin_bit not 0), and (0, 32) at 70,001; the patterns
there are uniform keys, three distinct keys and one digit per 64-key row.  minmax_keys_dev runs 64
columns up to n = 70,001 and 1 and 3 columns at n = 2,097,155 (64 columns of that length are half
a gigabyte, and the column count only sets gridDim.y)."""
import numpy as np
import pytest
import torch

import splat_hip as sh

pytestmark = pytest.mark.gpu

ST_ERR_ARG, ST_ERR_INTERNAL = -1, -7
GUARD = 64  # bytes, a multiple of 16: a buffer's alignment is its skew's
FILL = 0xA5
SS_MAX, TILE = 2048, 4096


@pytest.fixture(scope='module')
def ctx():
    c = sh.Context(0)
    c.bind_torch_stream(0)  # the tests' torch fills and copies are ordered with the library's kernels
    yield c
    c.close()


class Buf:
    """an array on the device between sentinel bytes, starting `skew` bytes past a 16-byte boundary"""

    def __init__(self, data, skew=0):
        data = np.ascontiguousarray(data)
        self.dtype, self.n, self.nbytes = data.dtype, len(data), data.nbytes
        self.lo = GUARD + skew
        self.t = torch.full((self.lo + self.nbytes + GUARD,), FILL, dtype=torch.uint8, device='cuda')
        assert self.t.data_ptr() % 16 == 0
        if self.nbytes:
            self.t[self.lo:self.lo + self.nbytes].copy_(torch.from_numpy(data.view(np.uint8).copy()))
        self.ptr = self.t.data_ptr() + self.lo

    @classmethod
    def empty(cls, n, dtype=np.uint32, skew=0):
        """n elements of sentinel bytes"""
        return cls(np.full(n, FILL, np.uint8).repeat(np.dtype(dtype).itemsize).view(dtype), skew)

    def read(self):
        """the contents; the sentinels on either side must be intact"""
        h = self.t.cpu().numpy()
        assert (h[:self.lo] == FILL).all() and (h[self.lo + self.nbytes:] == FILL).all(), 'a sentinel was overwritten'
        return h[self.lo:self.lo + self.nbytes].copy().view(self.dtype)


def refused(ctx, code, op, **kw):
    with pytest.raises(sh.StError) as e:
        ctx.dev_probe(op, **kw)
    assert e.value.code == code, e.value


# ---- scan ---------------------------------------------------------------------------------------------
SCAN_N = [0, 1, 7, 8, 9, 2047, 2048, 2049, 4096, 2048 ** 2 - 1, 2048 ** 2, 2048 ** 2 + 1]


def scan_values(n):
    rng = np.random.default_rng(n + 1)
    last = np.zeros(n, np.uint32)
    last[-1:] = 0xFFFFFFF0
    return {'ones': np.ones(n, np.uint32), 'flags': rng.integers(0, 2, n).astype(np.uint32),
            'wrapping': rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), 'last_only': last}


@pytest.mark.parametrize('n', SCAN_N)
def test_scan_matches_cumsum_mod_2_32(ctx, n):
    for name, v in scan_values(n).items():
        c = np.cumsum(v.astype(np.uint64))
        want = np.concatenate([np.zeros(1, np.uint64), c[:-1]]) & np.uint64(0xFFFFFFFF) if n else c
        total = int(c[-1]) & 0xFFFFFFFF if n else 0
        for in_place in (False, True):
            for where in ('null', 'separate', 'after_out'):
                tail = [FILL * 0x01010101] if where == 'after_out' else []
                out = Buf(np.concatenate([v if in_place else np.full(n, FILL * 0x01010101, np.uint32),
                                          np.array(tail, np.uint32)]).astype(np.uint32))
                src = out if in_place else Buf(v)
                sep = Buf.empty(1)
                aux = {'null': None, 'separate': sep.ptr, 'after_out': out.ptr + 4 * n}[where]
                ctx.dev_probe('scan', in0=src.ptr, out0=out.ptr, aux=aux, n=n)
                got = out.read()
                what = (name, in_place, where)
                assert np.array_equal(got[:n], want.astype(np.uint32)), what
                if where == 'after_out':
                    assert got[n] == total, what
                got_sep = sep.read()
                assert got_sep[0] == (total if where == 'separate' else FILL * 0x01010101), what
                if not in_place:
                    assert np.array_equal(src.read(), v), what


# ---- sorts --------------------------------------------------------------------------------------------
U32_N = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 2047, 2048, 2049, 4095, 4096, 4097, 8193, 70_001, 1_048_583]
U64_N = [0, 1, 2, 256, 257, 2048, 2049, 4097, 70_001]
U32_RANGES = [(0, 32), (0, 30), (0, 1), (0, 8), (0, 9), (0, 17), (3, 11), (7, 32), (5, 5), (21, 30)]
U64_RANGES = [(0, 64), (0, 33), (0, 40), (21, 42), (42, 63), (32, 64), (63, 64)]
PATTERNS = ['uniform', 'three', 'equal', 'ascending', 'descending', 'lane', 'row']
BIG_RANGES = {70_001: [(3, 11), (0, 9), (0, 17), (7, 32), (0, 32)], 1_048_583: [(3, 11), (0, 9), (0, 17), (7, 32)]}
BIG_PATTERNS = ['uniform', 'three', 'row']


def keys_of(pattern, n, width, b0, b1, rng):
    """n keys of `width` bits; the patterns that speak of digits put them at begin_bit and fill every other
    bit at random, so bits outside the range are there to be ignored"""
    dt = np.uint32 if width == 32 else np.uint64
    full = rng.integers(0, 1 << width, n, dtype=np.uint64, endpoint=False) if width < 64 else \
        rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    if pattern == 'uniform':
        k = full
    elif pattern == 'three':
        k = full[:3][rng.integers(0, 3, n)] if n >= 3 else full
    elif pattern == 'equal':
        k = np.full(n, full[0] if n else 0, np.uint64)
    elif pattern == 'ascending':
        k = np.sort(full)
    elif pattern == 'descending':
        k = np.sort(full)[::-1]
    else:
        i = np.arange(n, dtype=np.uint64)
        digit = (i % np.uint64(64)) if pattern == 'lane' else ((i // np.uint64(64)) % np.uint64(256))
        field = ((np.uint64(1) << np.uint64(b1 - b0)) - np.uint64(1)) << np.uint64(b0) if b1 - b0 < 64 else ~np.uint64(0)
        k = (full & ~field) | ((digit << np.uint64(b0)) & field)
    return np.ascontiguousarray(k).astype(dt)


def stable_order(k, b0, b1):
    bits = b1 - b0
    mask = np.uint64((1 << bits) - 1)
    return np.argsort((k.astype(np.uint64) >> np.uint64(b0)) & mask, kind='stable')


def passes_of(b0, b1):
    return (b1 - b0 + 7) // 8


def sort_cases(n, width):
    ranges = BIG_RANGES.get(n, U32_RANGES if width == 32 else U64_RANGES) if width == 32 else U64_RANGES
    patterns = BIG_PATTERNS if (width == 32 and n in BIG_RANGES) else PATTERNS
    rng = np.random.default_rng(n * 64 + width)
    for b0, b1 in ranges:
        for pattern in patterns:
            k = keys_of(pattern, n, width, b0, b1, rng)
            v = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)  # not a permutation of indices
            yield (b0, b1, pattern), k, v, stable_order(k, b0, b1)


def test_sort_pass_counts_cover_odd_and_even():
    assert sorted({passes_of(*r) for r in U32_RANGES}) == [0, 1, 2, 3, 4]
    for n, ranges in BIG_RANGES.items():
        assert {passes_of(*r) for r in ranges} >= {1, 2, 3, 4}
    assert {passes_of(*r) & 1 for r in U64_RANGES} == {0, 1}


@pytest.mark.parametrize('n', U32_N)
def test_radix_sort_u32_in_place(ctx, n):
    """radix_sort_u32, the key buffer on a 16-byte boundary and 4 bytes past one (k_rs_hist's quads / scalar reads)"""
    for what, k, v, order in sort_cases(n, 32):
        for skew in (0, 4):
            keys, vals = Buf(k, skew), Buf(v)
            ctx.dev_probe('sort_u32', out0=keys.ptr, out1=vals.ptr, n=n, begin_bit=what[0], end_bit=what[1])
            assert np.array_equal(keys.read(), k[order]), (what, skew)
            assert np.array_equal(vals.read(), v[order]), (what, skew)


@pytest.mark.parametrize('n', U32_N)
def test_radix_sort_u32_from(ctx, n):
    """radix_sort_u32_from: out of place (the input unchanged), with NULL values (the identity), in place
    with an even pass count, and refused in place with an odd one"""
    for what, k, v, order in sort_cases(n, 32):
        b0, b1 = what[0], what[1]
        for skew in (0, 4):
            src_k, src_v, out_k, out_v = Buf(k, skew), Buf(v), Buf.empty(n), Buf.empty(n)
            ctx.dev_probe('sort_from', in0=src_k.ptr, in1=src_v.ptr, out0=out_k.ptr, out1=out_v.ptr, n=n,
                          begin_bit=b0, end_bit=b1)
            assert np.array_equal(out_k.read(), k[order]) and np.array_equal(out_v.read(), v[order]), (what, skew)
            assert np.array_equal(src_k.read(), k) and np.array_equal(src_v.read(), v), (what, skew, 'input changed')
        src_k, out_k, out_v = Buf(k), Buf.empty(n), Buf.empty(n)
        ctx.dev_probe('sort_from', in0=src_k.ptr, in1=None, out0=out_k.ptr, out1=out_v.ptr, n=n, begin_bit=b0, end_bit=b1)
        assert np.array_equal(out_k.read(), k[order]) and np.array_equal(out_v.read(), order.astype(np.uint32)), what
        assert np.array_equal(src_k.read(), k), (what, 'input changed')
        # in place: both pairs, the keys alone, the values alone
        for alias_k, alias_v in ((True, True), (True, False), (False, True)):
            io_k, io_v = Buf(k), Buf(v)
            o_k, o_v = (io_k if alias_k else Buf.empty(n)), (io_v if alias_v else Buf.empty(n))
            args = dict(in0=io_k.ptr, in1=io_v.ptr, out0=o_k.ptr, out1=o_v.ptr, n=n, begin_bit=b0, end_bit=b1)
            if n and passes_of(b0, b1) & 1:
                refused(ctx, ST_ERR_INTERNAL, 'sort_from', **args)
                assert np.array_equal(io_k.read(), k) and np.array_equal(io_v.read(), v), (what, 'written')
                for o in (o_k, o_v):
                    if o not in (io_k, io_v):
                        assert (o.read().view(np.uint8) == FILL).all(), (what, 'written')
            else:
                ctx.dev_probe('sort_from', **args)
                assert np.array_equal(o_k.read(), k[order]) and np.array_equal(o_v.read(), v[order]), (what, alias_k, alias_v)


@pytest.mark.parametrize('n', U32_N)
def test_radix_sort_u32_iota_and_swap(ctx, n):
    for what, k, v, order in sort_cases(n, 32):
        b0, b1 = what[0], what[1]
        src_k, out_k, out_v = Buf(k), Buf.empty(n), Buf.empty(n)
        ctx.dev_probe('sort_iota', in0=src_k.ptr, out0=out_k.ptr, out1=out_v.ptr, n=n, begin_bit=b0, end_bit=b1)
        assert np.array_equal(out_k.read(), k[order]) and np.array_equal(out_v.read(), order.astype(np.uint32)), what
        assert np.array_equal(src_k.read(), k), (what, 'input changed')
        # _inplace_or_swap: the result stays in the caller's pair unless the tiled passes ran an odd number of times
        io_k, io_v, out_k, out_v = Buf(k), Buf(v), Buf.empty(n), Buf.empty(n)
        mine = ctx.dev_probe('sort_swap', in0=io_k.ptr, in1=io_v.ptr, out0=out_k.ptr, out1=out_v.ptr, n=n,
                             begin_bit=b0, end_bit=b1)
        assert np.array_equal(out_k.read(), k[order]) and np.array_equal(out_v.read(), v[order]), what
        assert mine == (0 if n > SS_MAX and passes_of(b0, b1) & 1 else 1), what
        if mine:
            assert np.array_equal(io_k.read(), k[order]) and np.array_equal(io_v.read(), v[order]), what
        else:
            io_k.read(), io_v.read()  # the sentinels


def test_swap_takes_both_outcomes():
    big = [n for n in U32_N if n > SS_MAX]
    assert big and {passes_of(*r) & 1 for r in U32_RANGES if r[0] != r[1]} == {0, 1}


@pytest.mark.parametrize('n', U64_N)
def test_radix_sort_u64(ctx, n):
    for what, k, v, order in sort_cases(n, 64):
        keys, vals = Buf(k), Buf(v)
        ctx.dev_probe('sort_u64', out0=keys.ptr, out1=vals.ptr, n=n, begin_bit=what[0], end_bit=what[1])
        assert np.array_equal(keys.read(), k[order]), what
        assert np.array_equal(vals.read(), v[order]), what


def test_sorts_refuse_bad_arguments(ctx):
    k, v, k64 = Buf(np.arange(16, dtype=np.uint32)), Buf(np.arange(16, dtype=np.uint32)), Buf(np.arange(16, dtype=np.uint64))
    o_k, o_v = Buf.empty(16), Buf.empty(16)
    for b0, b1 in ((0, 33), (-1, 8), (9, 8), (32, 40)):
        refused(ctx, ST_ERR_ARG, 'sort_u32', out0=k.ptr, out1=v.ptr, n=16, begin_bit=b0, end_bit=b1)
        refused(ctx, ST_ERR_ARG, 'sort_from', in0=k.ptr, in1=v.ptr, out0=o_k.ptr, out1=o_v.ptr, n=16, begin_bit=b0, end_bit=b1)
        refused(ctx, ST_ERR_ARG, 'sort_iota', in0=k.ptr, out0=o_k.ptr, out1=o_v.ptr, n=16, begin_bit=b0, end_bit=b1)
        refused(ctx, ST_ERR_ARG, 'sort_swap', in0=k.ptr, in1=v.ptr, out0=o_k.ptr, out1=o_v.ptr, n=16, begin_bit=b0, end_bit=b1)
    for b0, b1 in ((0, 65), (-1, 8), (40, 39)):
        refused(ctx, ST_ERR_ARG, 'sort_u64', out0=k64.ptr, out1=v.ptr, n=16, begin_bit=b0, end_bit=b1)
    refused(ctx, ST_ERR_ARG, 'sort_u64', out0=k64.ptr + 4, out1=v.ptr, n=8, begin_bit=0, end_bit=64)
    refused(ctx, ST_ERR_ARG, 'sort_u32', out0=k.ptr + 2, out1=v.ptr, n=8, begin_bit=0, end_bit=32)
    refused(ctx, ST_ERR_ARG, 'sort_u32', out0=k.ptr, out1=None, n=8, begin_bit=0, end_bit=32)
    refused(ctx, ST_ERR_ARG, 'sort_u32', out0=k.ptr, out1=v.ptr, n=1 << 32, begin_bit=0, end_bit=32)
    refused(ctx, ST_ERR_ARG, 'scan', in0=k.ptr, out0=o_k.ptr + 1, n=8)
    refused(ctx, ST_ERR_ARG, 'scan', in0=k.ptr, out0=o_k.ptr, aux=o_v.ptr + 2, n=8)
    refused(ctx, ST_ERR_ARG, 'scan', in0=k.ptr, out0=o_k.ptr, n=1 << 32)
    refused(ctx, ST_ERR_ARG, 'iota', out0=o_k.ptr + 2, n=8)
    for b in (k, v, k64):
        assert np.array_equal(b.read(), np.arange(16))
    for b in (o_k, o_v):
        assert (b.read().view(np.uint8) == FILL).all()


# ---- min / max ------------------------------------------------------------------------------------------
MM_N = [0, 1, 3, 4, 5, 1023, 4096, 4097, 70_001, 2_097_155]
MM_SETS = ['nans', 'all_nan', 'zeros', 'infs', 'subnormals', 'ends']
MM_BLOCKS = 512


def mm_values(kind, n, rng):
    if kind == 'nans':
        v = rng.normal(0, 100, n).astype(np.float32)
        nan = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff812345], np.uint32).view(np.float32)
        return np.where(rng.random(n) < 0.1, nan[rng.integers(0, 4, n)], v)
    if kind == 'all_nan':
        return np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xffffffff], np.uint32).view(np.float32)[rng.integers(0, 4, n)]
    if kind == 'zeros':
        return np.where(rng.random(n) < 0.5, np.float32(-0.0), np.float32(0.0))
    if kind == 'infs':
        v = rng.normal(0, 1e30, n).astype(np.float32)
        return np.where(rng.random(n) < 0.01, np.where(rng.random(n) < 0.5, np.float32(np.inf), np.float32(-np.inf)), v)
    if kind == 'subnormals':
        return (rng.integers(1, 1 << 23, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31)).view(np.float32)
    # the minimum in the last element, the maximum in the first element of the last slice a workgroup takes
    v = rng.uniform(-1, 1, n).astype(np.float32)
    if n:
        nb = max(1, min(MM_BLOCKS, (n + 4095) // 4096))
        per = ((n + nb - 1) // nb + 3) & ~3
        v[((n - 1) // per) * per] = 7.0
        if n > 1:
            v[n - 1] = -5.0
    return v


def mm_reference(v):
    u = v[~np.isnan(v)].view(np.uint32)
    if not len(u):
        return 0xFFFFFFFF, 0
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return int(key.min()), int(key.max())


@pytest.mark.parametrize('n', MM_N)
def test_minmax_keys(ctx, n):
    rng = np.random.default_rng(n + 7)
    for ncols in ((1, 3) if n > 70_001 else (1, 3, 64)):
        # a column's value set and its start (0, 4, 8, 12 bytes past a 16-byte boundary) both go round with its
        # index; the shifts bring every set to every start for one column, every set to every column for three
        shifts = [(a, b) for a in range(6) for b in range(4)] if ncols == 1 else [(a, a) for a in range(6)] if ncols == 3 \
            else [(0, 0)]
        for sa, sb in shifts:
            cols = [mm_values(MM_SETS[(j + sa) % 6], n, rng) for j in range(ncols)]
            bufs = [Buf(c, 4 * ((j + sb) % 4)) for j, c in enumerate(cols)]
            out = Buf.empty(2 * ncols)
            ctx.dev_probe('minmax', cols=[b.ptr for b in bufs], out0=out.ptr, n=n)
            got = out.read().reshape(ncols, 2)
            for j, c in enumerate(cols):
                assert (int(got[j, 0]), int(got[j, 1])) == mm_reference(c), (ncols, sa, sb, j, MM_SETS[(j + sa) % 6])


def test_minmax_key_order_and_column_limit(ctx):
    v = np.array([0.0, -0.0], np.float32)
    assert mm_reference(v) == (0x7FFFFFFF, 0x80000000)  # -0 < +0
    assert mm_reference(np.array([np.nan], np.float32)) == (0xFFFFFFFF, 0)
    col, out = Buf(np.ones(8, np.float32)), Buf.empty(2 * 65)
    refused(ctx, ST_ERR_ARG, 'minmax', cols=[col.ptr] * 65, out0=out.ptr, n=8)
    refused(ctx, ST_ERR_ARG, 'minmax', cols=[], out0=out.ptr, n=8)
    refused(ctx, ST_ERR_ARG, 'minmax', cols=[col.ptr + 2], out0=out.ptr, n=4)
    assert (out.read().view(np.uint8) == FILL).all()


# ---- iota -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [0, 1, 4097, 1_048_583])
def test_iota(ctx, n):
    out = Buf.empty(n)
    ctx.dev_probe('iota', out0=out.ptr, n=n)
    assert np.array_equal(out.read(), np.arange(n, dtype=np.uint32))
