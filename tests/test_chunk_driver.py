"""The host side the verification scores share, without a device: the buffer scope of dl4ds_amd/device.py, the chunk driver and the band driver of
dl4ds_amd/_chunks.py and the exact ratios of dl4ds_amd/_exact.py.  A stub stands in for the library: device memory is host memory."""
import ctypes
import gc
import random
from fractions import Fraction

import numpy as np
import pytest


class StubLib:
    """dl4ds_malloc / free / memset / memcpy over ctypes buffers; every call is counted, every copy checked against the bounds of
    a live buffer and logged as (buffer address, byte offset, the bytes)."""

    def __init__(self):
        self.live, self.frees, self.n_malloc = {}, {}, 0
        self.h2d, self.d2h = [], []

    def _inside(self, ptr, n):
        for base, buf in self.live.items():
            if base <= ptr and ptr + n <= base + len(buf):
                return base
        raise AssertionError(f'{n} bytes at {ptr:#x} lie in no live buffer')

    def dl4ds_malloc(self, out, nbytes):
        buf = ctypes.create_string_buffer(b'\xa5' * nbytes, nbytes)
        out._obj.value = ctypes.addressof(buf)
        self.live[out._obj.value] = buf
        self.n_malloc += 1
        return 0

    def dl4ds_free(self, ptr):
        self.frees[ptr] = self.frees.get(ptr, 0) + 1
        self.live.pop(ptr, None)
        return 0

    def dl4ds_memset(self, ptr, value, n):
        self._inside(ptr, n)
        ctypes.memset(ptr, value, n)
        return 0

    def dl4ds_memcpy_h2d(self, dst, src, n):
        base = self._inside(dst, n)
        ctypes.memmove(dst, src, n)
        self.h2d.append((base, dst - base, ctypes.string_at(src, n)))
        return 0

    def dl4ds_memcpy_d2h(self, dst, src, n):
        base = self._inside(src, n)
        ctypes.memmove(dst, src, n)
        self.d2h.append((base, src - base, n))
        return 0


@pytest.fixture
def stub(monkeypatch):
    import dl4ds_amd._lib as L
    s = StubLib()
    monkeypatch.setattr(L, 'lib', lambda: s)
    return s


def test_buffer_scope_frees_every_buffer_once(stub):
    from dl4ds_amd._chunks import paired_chunks
    from dl4ds_amd.device import Buffers
    with Buffers() as buf:
        held = [buf.alloc((3, 2)), buf.zeros((5,), np.int64), buf.alloc((4,), np.float64), buf.alloc((0,))]
        ptrs = [d.ptr for d in held]
        assert len(set(ptrs)) == 4 and set(ptrs) == set(stub.live) and not stub.frees
        held[2].upload(np.arange(2, dtype=np.float64), offset=1)
        back = np.empty(2)
        held[2].download(back, offset=1)
        assert bytes(stub.live[ptrs[1]]) == bytes(40) and stub.h2d == [(ptrs[2], 8, np.arange(2, dtype=np.float64).tobytes())]
        assert stub.d2h == [(ptrs[2], 8, 16)] and back.tolist() == [0.0, 1.0]
    assert stub.frees == {p: 1 for p in ptrs} and not stub.live and all(d.ptr is None for d in held)
    del held, buf
    gc.collect()
    assert stub.frees == {p: 1 for p in ptrs}, 'a freed buffer is not freed again when it is collected'

    class Boom(Exception):
        pass

    def call(b, *ptrs):
        assert len(stub.live) == 4                     # observation, prediction, two outputs
        raise Boom
    y = np.zeros((7, 3, 2, 1), np.float32)
    stub.frees.clear()
    before = stub.n_malloc
    with pytest.raises(Boom):
        paired_chunks(y, y, (np.empty((7, 2), np.int64), np.empty((7,), np.float64)), call, batch_size=2)
    assert stub.n_malloc - before == 4 and sorted(stub.frees.values()) == [1, 1, 1, 1] and not stub.live
    stub.frees.clear()                                 # (the host allocator may hand the same address out again)

    class Owned:                                       # what `own` takes over: anything with a free(), a scorer for one
        freed = 0

        def free(self):
            self.freed += 1
    with pytest.raises(Boom):                          # the scope alone, an exception passing through
        with Buffers() as buf:
            p, other = buf.alloc((2,)).ptr, buf.own(Owned())
            raise Boom
    assert stub.frees[p] == 1 and not stub.live and other.freed == 1


def _check_coverage(stub, axis, shape, with_pred):
    """7 units along `axis`: each goes up and comes back once, in ascending order, for every chunk size"""
    from dl4ds_amd._chunks import paired_chunks, upload_batch
    rng = np.random.default_rng(3)
    obs = rng.standard_normal(shape).astype(np.float32)
    obs[1, 2, 0, 1] = np.nan
    pred = rng.standard_normal(shape) if with_pred else None               # float64: the driver makes it float32
    units, per = 7, obs.size // 7
    assert upload_batch(None, per, units) == 7 and upload_batch(None, 1 << 25, units) == 2 and upload_batch(None, 1 << 27, units) == 1
    want_a = np.arange(units * 2, dtype=np.int64).reshape(units, 2) * 3 + 1               # one row per unit
    want_b = np.arange(units * 3, dtype=np.float64) / 7.0                                   # three rows per unit
    for batch_size in (1, 2, 3, 7, 8, None):
        bmax = min(batch_size or units, units)
        chunks = [(i, min(bmax, units - i)) for i in range(0, units, bmax)]
        del stub.h2d[:], stub.d2h[:]
        stub.frees.clear()
        out_a, out_b = np.full((units, 2), -1, np.int64), np.full((units * 3,), np.nan)
        seen = []

        def call(b, y_ptr, p_ptr, a_ptr, b_ptr):
            i = sum(n for _, n in seen)
            seen.append((i, b))
            take = (slice(None),) * axis + (slice(i, i + b),)
            assert ctypes.string_at(y_ptr, b * per * 4) == np.ascontiguousarray(obs[take]).tobytes(), 'byte for byte'
            if with_pred:
                assert ctypes.string_at(p_ptr, b * per * 4) == np.ascontiguousarray(pred[take], np.float32).tobytes()
            else:
                assert p_ptr is None
            ctypes.memmove(a_ptr, want_a[i:i + b].ctypes.data, b * 2 * 8)
            ctypes.memmove(b_ptr, want_b[3 * i:3 * (i + b)].ctypes.data, b * 3 * 8)
        paired_chunks(obs, pred, (out_a, out_b), call, batch_size, axis)
        assert seen == chunks, 'ascending, every unit once'
        np.testing.assert_array_equal(out_a, want_a)
        np.testing.assert_array_equal(out_b, want_b)
        n_in = 2 if with_pred else 1
        assert len(stub.h2d) == n_in * len(chunks) and len(stub.d2h) == 2 * len(chunks)
        assert len({base for base, _, _ in stub.h2d}) == n_in, 'nothing is uploaded for a missing prediction'
        assert all(off == 0 for _, off, _ in stub.h2d) and all(off == 0 for _, off, _ in stub.d2h)
        for (i, b), (_, _, sent) in zip(chunks, stub.h2d[::n_in]):
            assert sent == np.ascontiguousarray(obs[(slice(None),) * axis + (slice(i, i + b),)]).tobytes()
        assert sum(n for _, _, n in stub.d2h) == out_a.nbytes + out_b.nbytes, 'every output row is downloaded once'
        assert sorted(stub.frees.values()) == [1] * (n_in + 2) and not stub.live


def test_chunk_driver_covers_every_unit_once_in_order(stub):
    from dl4ds_amd._chunks import paired_chunks
    for axis, shape in ((0, (7, 5, 3, 2)), (1, (5, 7, 3, 2))):             # samples; the row bands of over='time'
        for with_pred in (True, False):
            _check_coverage(stub, axis, shape, with_pred)
    del stub.d2h[:]                                                        # an output of zero bytes is not transferred
    y = np.zeros((3, 2, 2, 1), np.float32)
    empty, full = np.empty((3, 2, 0), np.float64), np.empty((3,), np.int64)
    paired_chunks(y, y, (empty, full), lambda b, *ptrs: None, batch_size=2)
    assert [n for _, _, n in stub.d2h] == [16, 8]


# ---------------------------------------------------------------------------------------------------------- the band driver
GRID = (4, 5, 3, 2)                                    # N, H, W, C: bands of 2 grid rows leave a ragged last band of one


def _bands(batch_size):
    """[(cells, c0)] that `cell_bands` must hand out on GRID"""
    _, H, W, C = GRID
    b = min(batch_size or H, H)
    return [(min(b, H - i) * W * C, i * W * C) for i in range(0, H, b)]


def _fill(ptr, shape, dtype, c0):
    """writes cell index + 1000 * leading index into the device buffer [...][cells] at ``ptr``"""
    cells = shape[-1]
    lead = np.arange(int(np.prod(shape[:-1], dtype=np.int64))).reshape(shape[:-1] + (1,))
    want = np.ascontiguousarray((c0 + np.arange(cells)) + 1000 * lead, dtype)
    ctypes.memmove(ptr, want.ctypes.data, want.nbytes)


def _expected(shape, dtype):
    per = shape[-1]
    lead = np.arange(int(np.prod(shape[:-1], dtype=np.int64))).reshape(shape[:-1] + (1,))
    return (np.arange(per) + 1000 * lead).astype(dtype)


@pytest.mark.parametrize('batch_size', [2, 5, None])
def test_cell_bands_cover_every_cell_once_and_place_the_outputs(stub, batch_size):
    from dl4ds_amd._chunks import cell_bands
    N, H, W, C = GRID
    per = H * W * C
    rng = np.random.default_rng(5)
    x = rng.integers(-300, 300, GRID).astype(np.int16)                     # goes up as its float32 conversion
    pred = rng.standard_normal(GRID)
    field = rng.standard_normal((3,) + GRID[1:]).astype(np.float32)        # per cell: cut per band
    flat = np.arange(3, dtype=np.float32)                                  # (T,): uploaded once
    empty = np.zeros((0,), np.float32)
    outs = [np.full((per,), -1, np.int32), None, np.full((2, per), -1, np.int64), np.full((3, 2, per), np.nan, np.float64)]
    seen = []

    def call(band):
        seen.append((band.cells, band.c0))
        rows = slice(band.c0 // (W * C), (band.c0 + band.cells) // (W * C))
        assert ctypes.string_at(band.x, N * band.cells * 4) == np.ascontiguousarray(x[:, rows], np.float32).tobytes()
        assert ctypes.string_at(band.pred, N * band.cells * 4) == np.ascontiguousarray(pred[:, rows], np.float32).tobytes()
        assert ctypes.string_at(band.fields[0], 3 * band.cells * 4) == np.ascontiguousarray(field[:, rows]).tobytes(), 'cell order'
        assert ctypes.string_at(band.fields[1], 12) == flat.tobytes() and band.fields[2] is None
        assert band.outs[1] is None
        for h, ptr in zip(outs, band.outs):
            if h is not None:
                _fill(ptr, h.shape[:-1] + (band.cells,), h.dtype, band.c0)
    cell_bands(x, pred, GRID, outs, call, batch_size, fields=(field, flat, empty))
    want = _bands(batch_size)
    assert seen == want and (batch_size != 2 or want == [(12, 0), (12, 12), (6, 24)]), 'ascending, every cell once'
    for h in (outs[0], outs[2], outs[3]):
        np.testing.assert_array_equal(h, _expected(h.shape, h.dtype))
    # two inputs, three outputs, two fields: allocated once at the widest band, every one freed exactly once
    assert stub.n_malloc == 7 and sorted(stub.frees.values()) == [1] * 7 and not stub.live
    flat_uploads = [sent for _, _, sent in stub.h2d if sent == flat.tobytes()]
    assert len(flat_uploads) == 1 and len(stub.h2d) == 3 * len(want) + 1
    assert sum(n for _, _, n in stub.d2h) == sum(h.nbytes for h in outs if h is not None), 'every output column comes back once'


def test_cell_bands_upload_dtype(stub):
    from dl4ds_amd._chunks import cell_bands
    x = np.random.default_rng(6).standard_normal(GRID)                     # float64 stays float64 when asked for
    n = np.empty((GRID[1] * GRID[2] * GRID[3],), np.int32)
    cell_bands(x, None, GRID, (n,), lambda band: _fill(band.outs[0], (band.cells,), np.int32, band.c0), 2, dtype=np.float64)
    assert [sent for _, _, sent in stub.h2d] == [np.ascontiguousarray(x[:, i:i + 2]).tobytes() for i in (0, 2, 4)]
    np.testing.assert_array_equal(n, np.arange(n.size))
    del stub.h2d[:]
    ints = np.arange(np.prod(GRID), dtype=np.int16).reshape(GRID)
    cell_bands(ints, None, GRID, (n,), lambda band: None, 5)
    assert [sent for _, _, sent in stub.h2d] == [ints.astype(np.float32).tobytes()]


def test_cell_bands_free_every_buffer_also_when_the_call_raises(stub):
    from dl4ds_amd._chunks import cell_bands

    class Boom(Exception):
        pass
    x = np.zeros(GRID, np.float32)
    out = np.empty((2, GRID[1] * GRID[2] * GRID[3]), np.float64)
    extra = []

    def call(band):
        extra.append(band.buf.alloc((3, band.cells)).ptr)                  # a second phase allocates from the band's scope
        assert extra[-1] in stub.live
        if len(extra) > 1:
            assert extra[0] not in stub.live or extra[0] == extra[-1], 'the first band\'s buffer went with its band'
        if len(extra) == 2:
            raise Boom
    with pytest.raises(Boom):
        cell_bands(x, None, GRID, (out,), call, 2)
    assert stub.n_malloc == 4 and sum(stub.frees.values()) == 4 and not stub.live
    stub.frees.clear()
    del extra[:]
    before = stub.n_malloc
    cell_bands(x, None, GRID, (out,), lambda band: extra.append(band.buf.alloc((band.cells,)).ptr), 2)
    assert stub.n_malloc - before == 2 + 3 and sum(stub.frees.values()) == 5 and not stub.live


def test_cell_bands_device_array_in_one_call(stub):
    from dl4ds_amd._chunks import cell_bands
    from dl4ds_amd.device import DeviceArray
    per = GRID[1] * GRID[2] * GRID[3]
    x = DeviceArray(GRID)
    field = np.arange(2 * per, dtype=np.float32).reshape((2,) + GRID[1:])
    out = np.empty((2, per), np.int64)
    seen = []

    def call(band):
        seen.append((band.cells, band.c0, band.x))
        assert ctypes.string_at(band.fields[0], field.nbytes) == field.tobytes()
        _fill(band.outs[0], (2, band.cells), np.int64, band.c0)
    cell_bands(x, None, GRID, (out,), call, 2, fields=(field,))
    assert seen == [(per, 0, x.ptr)] and len(stub.h2d) == 1, 'one call over all cells; nothing of the input is uploaded'
    np.testing.assert_array_equal(out, _expected(out.shape, np.int64))
    assert x.ptr in stub.live and len(stub.live) == 1, 'the caller\'s array is not the driver\'s to free'
    x.free()


def test_exact_ratios_against_fractions():
    from dl4ds_amd import _exact
    rnd = random.Random(11)
    nan = float('nan')
    ranges = [(0, 2 ** 53 - 1), (2 ** 53, 2 ** 63 - 1), (2 ** 64, 2 ** 200)]
    for lo, hi in ranges:
        num = [rnd.randint(lo, hi) for _ in range(40)] + [lo, hi, 0, hi]
        den = [rnd.randint(max(lo, 1), hi) for _ in range(40)] + [hi, max(lo, 1), hi, 0]
        want = [float(Fraction(n, d)) if d else nan for n, d in zip(num, den)]
        for n, d, w in zip(num, den, want):
            got = _exact.int_ratio(n, d)
            assert got == w or (d == 0 and got != got), (n, d)
        np.testing.assert_array_equal(_exact.ratio_exact(np.array(num, object), np.array(den, object)), np.array(want))
        if hi < 2 ** 63:
            n64, d64 = np.array(num, np.int64), np.array(den, np.int64)
            np.testing.assert_array_equal(_exact.quotient(n64, d64), np.array(want), err_msg='quotient picks a branch that rounds once')
            np.testing.assert_array_equal(_exact.quotient(n64.astype(object), d64), np.array(want))
        if hi < 2 ** 53:
            np.testing.assert_array_equal(_exact.ratio(np.array(num, np.int64), np.array(den, np.int64)), np.array(want),
                                          err_msg='operands below 2^53 are exact in fp64: one IEEE division is the correctly rounded quotient')
    assert np.isnan(_exact.ratio(3, 0)) and np.isnan(_exact.quotient(np.array([3]), np.array([0]))[0]) and _exact.quotient(np.zeros(0, np.int64), 1).size == 0
    assert _exact.ratio_exact(2 ** 70, 2 ** 69)[()] == 2.0 and np.isnan(_exact.ratio_exact(1, 0)[()])
    big = np.array([[2 ** 62, 2 ** 62], [2 ** 62, 1]], np.int64)
    assert _exact.pysum(big, (0, 1)) == 3 * 2 ** 62 + 1 and _exact.pysum(big, 0).tolist() == [2 ** 63, 2 ** 62 + 1]
    assert _exact.wide(big, 2 ** 62 - 1) is big and _exact.wide(big, 2 ** 62).dtype == object
