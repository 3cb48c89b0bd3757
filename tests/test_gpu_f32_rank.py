"""GPU: the order statistics (include/specan_rank.h: sa_rank_f32 of libspecan_rank.so), through SpectrumChain.order_stats,
SpectrumChain.noise_floor_f32 and the C entry point.

Every comparison is exact, on float bits, against the numpy mirror frames.ranks_of_rows, whose probes
tests/test_f32_rank_cpu.py works out by hand; the probes are part of the data here, and their expected bits are asserted
again on the device's.  One case is held to torch.sort of the keys on the device instead, a reference that shares nothing with
the mirror.

The kernel's ownership (csrc/rank_f32.hip) is that of the peak table: a row is dealt in 16-byte units, unit t + 256 j to
thread t; a unit is four bins of magnitudes (field 0) or two bins of records (fields 1, 2).  EDGES (of
tests/test_gpu_f32_peaks.py) holds the first and last bin on both sides of each lane, wave and unit boundary for both unit
sizes: a range that starts or ends there cuts a unit, a wave's units or a thread's registers in two."""
import ctypes

import numpy as np
import pytest

from conftest import N, load_golden
from gpu_support import ch, lds_fill, to_device, torch_mod  # noqa: F401 (fixtures)
from test_f32_rank_cpu import ONE, ONE_UP, SPECIALS, SPECIALS_TOP6
from test_gpu_f32_peaks import EDGES, _inputs, _tones

pytestmark = pytest.mark.gpu

SA_OK, SA_EINVAL, SA_ESHAPE = 0, -1, -2
FIELDS = (None, "peak", "power")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _records(pts, field):
    """``pts`` float32 [R, N] in the layout of ``field``: itself, or records whose other float is a NaN"""
    if field is None:
        return pts
    rec = np.full(pts.shape + (2,), np.nan, np.float32)
    rec[..., 0 if field == "peak" else 1] = pts
    return rec


def _stats(ch, torch, x, ranks, **kw):
    """order_stats on the device tensor -> its bits uint32 [R, q] on the host"""
    got = ch.order_stats(x, ranks, **kw)
    assert got.dtype == torch.float32 and tuple(got.shape) == (x.shape[0], len(ranks)) and got.is_contiguous()
    return _bits(got.cpu().numpy())


def _same(got, pts, ranks, tag, lo=0, hi=N):
    """the device's bits against the mirror's on the plain points"""
    from fpga_real_time_fft_analyzer_amd import frames
    want = _bits(frames.ranks_of_rows(pts, ranks, lo, hi))
    bad = np.nonzero(got != want)
    assert got.shape == want.shape and bad[0].size == 0, (tag, bad[0][:5], bad[1][:5], got[bad][:5], want[bad][:5])
    return want


def _rank_sets(m):
    """the rank sets of a range of m bins: the minimum, the maximum, five across it, and eight unsorted with repeats"""
    five = [0, min(1, m - 1), m // 2, max(m - 2, 0), m - 1]
    eight = [m - 1, 0, m // 3, m - 1, (2 * m) // 3, m // 3, min(7, m - 1), m // 2]
    return [0], [m - 1], five, eight


@pytest.fixture(scope="module")
def wide():
    """R = 3 rows of exp(uniform +-60): keys spread over 170 exponents, every bit of a key in play"""
    rng = np.random.default_rng(1810)
    return np.exp(rng.uniform(-60.0, 60.0, size=(3, N))).astype(np.float32)


@pytest.mark.parametrize("field", FIELDS)
def test_rank_sets_and_ranges_equal_the_mirror(ch, torch_mod, wide, field):
    """The full range, width 1 and width 2, and ranges that start or end at every ownership edge: each edge e as [e, N),
    [0, e) and [e, the next edge)."""
    x = to_device(torch_mod, _records(wide, field))
    ranges = [(0, N), (0, 1), (N - 1, N), (5000, 5001), (0, 2), (N - 2, N), (4095, 4097), (255, 257)]
    for i, e in enumerate(EDGES):
        ranges += [(e, N)] + ([(0, e)] if e else []) + ([(e, EDGES[i + 1])] if i + 1 < len(EDGES) else [])
    for lo, hi in ranges:
        for ranks in _rank_sets(hi - lo):
            _same(_stats(ch, torch_mod, x, ranks, lo=lo, hi=hi, field=field), wide, ranks, (field, lo, hi, ranks), lo, hi)


@pytest.mark.parametrize("field", FIELDS)
def test_hand_probes_on_the_device(ch, torch_mod, field):
    """The probes of tests/test_f32_rank_cpu.py with their expected bits, derived there; the last-bit probe (a row of 1.0 with
    one bin one ulp up) and a bit-30 probe (a zero row with 2.0 = 0x40000000 and, in the neighbouring bin, the denormal of bits
    1) planted at every bin of EDGES, one row each."""
    torch = torch_mod
    up = np.nextafter(np.float32(1), np.float32(2), dtype=np.float32)
    rows = np.ones((len(EDGES), N), np.float32)
    rows[np.arange(len(EDGES)), EDGES] = up
    got = _stats(ch, torch, to_device(torch, _records(rows, field)), [N - 1, N - 2, 0], field=field)
    assert (got == np.array([ONE_UP, ONE, ONE], np.uint32)).all(), (field, np.nonzero(got != np.array([ONE_UP, ONE, ONE]))[0])
    _same(got, rows, [N - 1, N - 2, 0], (field, "last bit"))
    rows = np.zeros((len(EDGES), N), np.float32)
    rows[np.arange(len(EDGES)), EDGES] = 2.0
    rows[np.arange(len(EDGES)), np.array(EDGES) ^ 1] = 1e-45
    got = _stats(ch, torch, to_device(torch, _records(rows, field)), [N - 1, N - 2, N - 3, 0], field=field)
    assert (got == np.array([0x40000000, 1, 0, 0], np.uint32)).all(), field
    _same(got, rows, [N - 1, N - 2, N - 3, 0], (field, "bit 30"))
    # the specials: NaN above +inf, -3.0 as 3.0, the denormal kept, -0.0 as zero
    pts = np.zeros((1, N), np.float32)
    for b, v in SPECIALS:
        pts[0, b] = v
    top6 = list(range(N - 6, N))
    got = _stats(ch, torch, to_device(torch, _records(pts, field)), top6, field=field)
    assert got[0].tolist() == SPECIALS_TOP6, field
    assert _stats(ch, torch, to_device(torch, _records(pts, field)), [0, N - 7], field=field)[0].tolist() == [0, 0]
    pts = np.zeros((1, N), np.float32)
    pts.view(np.uint32)[0, 77] = 0xFFC00123                       # a negative NaN: the sign cleared, the payload kept
    assert _stats(ch, torch, to_device(torch, _records(pts, field)), [N - 1, N - 2], field=field)[0].tolist() == [0x7FC00123, 0]
    # narrow ranges, repeated and unsorted ranks, and a huge value right outside the range
    pts = np.zeros((1, N), np.float32)
    pts[0, 500:503] = (5.0, 5.0, -7.0)
    x = to_device(torch, _records(pts, field))
    five, seven = 0x40A00000, 0x40E00000
    for ranks, lo, hi, want in (([0], 500, 501, [five]), ([0], 502, 503, [seven]), ([0], 499, 500, [0]), ([0, 1], 500, 502, [five, five]),
                                ([1, 0], 501, 503, [seven, five]), ([0, 1], 499, 501, [0, five])):
        assert _stats(ch, torch, x, ranks, lo=lo, hi=hi, field=field)[0].tolist() == want, (field, lo, hi)
    ramp = np.arange(N, dtype=np.float32)[None, :]
    ranks = [9000, 3, 9000, N - 1, 0, 3, 12345, 9000]
    got = _stats(ch, torch, to_device(torch, _records(ramp, field)), ranks, field=field)
    assert got[0].tolist() == _bits(np.array(ranks, np.float32)).tolist(), field
    loud = ramp.copy()
    loud[0, 999] = loud[0, 3000] = 3e38
    got = _stats(ch, torch, to_device(torch, _records(loud, field)), [0, 1999, 1000], lo=1000, hi=3000, field=field)
    assert got[0].tolist() == _bits(np.array([1000, 2999, 2000], np.float32)).tolist(), field


@pytest.mark.parametrize("field", FIELDS)
def test_massive_ties(ch, torch_mod, field):
    """Rows of the integers 0..3, a constant row and a zero row: the answer is decided by counts in the thousands that change
    by one bin."""
    rng = np.random.default_rng(1811)
    pts = rng.integers(0, 4, size=(5, N)).astype(np.float32)
    pts[3] = 7.25
    pts[4] = 0.0
    x = to_device(torch_mod, _records(pts, field))
    n = [(pts[0] == v).sum() for v in range(4)]
    edges = [int(e) for e in np.cumsum(n)]
    for ranks in ([0, edges[0] - 1, edges[0], edges[1] - 1, edges[1], edges[2] - 1, edges[2], N - 1], [N // 2], [0, N - 1]):
        got = _stats(ch, torch_mod, x, ranks, field=field)
        _same(got, pts, ranks, (field, ranks))
        assert (got[3] == 0x40E80000).all() and not got[4].any()
    got = _stats(ch, torch_mod, x, [edges[0] - 1, edges[0]], field=field)
    assert got[0].tolist() == [0, ONE]                            # the last zero and the first 1.0 of row 0
    for lo, hi in ((1, N - 1), (4097, 12289)):
        ranks = _rank_sets(hi - lo)[3]
        _same(_stats(ch, torch_mod, x, ranks, lo=lo, hi=hi, field=field), pts, ranks, (field, lo, hi), lo, hi)


def test_specials_in_wide_rows_and_rows_between_nan_rows(ch, torch_mod, wide):
    """R = 7: NaN rows around and between the data rows, an all-inf row; the data rows equal their single-row calls."""
    nan_row, inf_row = np.full((1, N), np.nan, np.float32), np.full((1, N), np.inf, np.float32)
    pts = np.concatenate([nan_row, wide[:1], nan_row, wide[1:2], inf_row, wide[2:], nan_row])
    pts[1, 4000] = np.nan
    pts[1, 9000] = -np.inf
    pts[3, 12000] = -0.0
    pts[5, 0] = np.inf
    pts[5, 1::2] *= -1.0
    ranks = [N - 1, N - 2, N - 3, 0, 1, N // 2, 100, N - 100]
    for field in FIELDS:
        x = to_device(torch_mod, _records(pts, field))
        got = _stats(ch, torch_mod, x, ranks, field=field)
        _same(got, pts, ranks, field)
        assert (got[[0, 2, 6]] == 0x7FC00000).all() and (got[4] == 0x7F800000).all()
        assert got[1, 0] == 0x7FC00000 and got[1, 1] == 0x7F800000 and got[3, 3] == 0 and got[5, 0] == 0x7F800000
        for r in (1, 3, 5):
            one = _stats(ch, torch_mod, x[r:r + 1], ranks, field=field)
            assert np.array_equal(one, got[r:r + 1]), (field, r)


def test_64_rows_against_torch_sort(ch, torch_mod):
    """R = 64, signs mixed: the keys sorted by torch.sort on the device, gathered at the ranks -- nothing of the mirror."""
    torch = torch_mod
    rng = np.random.default_rng(1812)
    pts = (np.exp(rng.uniform(-60.0, 60.0, size=(64, N))) * rng.choice([-1.0, 1.0], size=(64, N))).astype(np.float32)
    x = to_device(torch, pts)
    ranks = [8191, 0, N - 1, 4095, 12287, 1, N - 2, 8191]
    for lo, hi, rk in ((0, N, ranks), (1023, 9001, [v % (9001 - 1023) for v in ranks])):
        keys = (x.view(torch.int32) & 0x7FFFFFFF)[:, lo:hi]
        want = torch.sort(keys, dim=1).values[:, rk]
        got = ch.order_stats(x, rk, lo=lo, hi=hi)
        assert torch.equal(got.view(torch.int32), want), (lo, hi)
    rec = torch.stack([x, -x], dim=2).contiguous()
    want = torch.sort(x.view(torch.int32) & 0x7FFFFFFF, dim=1).values[:, ranks]
    assert torch.equal(ch.order_stats(rec, ranks, field="power").view(torch.int32), want)


def _c_ranks(values):
    return (ctypes.c_int32 * len(values))(*values)


def test_exactly_the_output_bytes_are_written_and_a_refused_call_writes_nothing(ch, torch_mod, wide):
    from fpga_real_time_fft_analyzer_amd import abi
    from fpga_real_time_fft_analyzer_amd.abi import SpecanError
    torch = torch_mod
    L = abi.rank_lib()
    stream = torch.cuda.current_stream().cuda_stream
    R, guard = 3, 4096
    x = to_device(torch, wide)
    for ranks in ([8191], [0, N - 1, 8191, 5, 5], [7, 6, 5, 4, 3, 2, 1, 0]):
        q = len(ranks)
        out = torch.full((R * q * 4 + guard,), 0xFF, dtype=torch.uint8, device="cuda")
        assert L.sa_rank_f32(x.data_ptr(), 0, out.data_ptr(), R, q, _c_ranks(ranks), 0, N, stream) == SA_OK
        assert L.sa_rank_last_error() == b""
        torch.cuda.synchronize()
        assert (out[R * q * 4:] == 0xFF).all().item()
        got = out[:R * q * 4].cpu().numpy().view(np.uint32).reshape(R, q)
        assert (got != 0xFFFFFFFF).all()                          # every word was written: no key is all ones
        _same(got, wide, ranks, ("C call", q))
    # refused calls: the code of sa_rank_check for the same arguments, its text, and nothing written
    q, ranks = 3, [0, 100, N - 1]
    out = torch.full((R * q * 4 + guard,), 0xFF, dtype=torch.uint8, device="cuda")
    flat = torch.zeros((R * N + 64,), dtype=torch.float32, device="cuda")
    before = flat.clone()
    p_in, p_out = flat.data_ptr(), out.data_ptr()
    for tag, args, code, words in (
            ("in 4 bytes off", (p_in + 4, 0, p_out, R, q, ranks, 0, N), SA_EINVAL, "`in` must be 16-byte aligned"),
            ("out 2 bytes off", (p_in, 0, p_out + 2, R, q, ranks, 0, N), SA_EINVAL, "`out` must be 4-byte aligned"),
            ("out inside in", (p_in, 0, p_in + R * N * 4 - 4, R, q, ranks, 0, N), SA_EINVAL, "overlap"),
            ("records read twice as much", (p_in, 2, p_in + R * N * 4, R, q, ranks, 0, N), SA_EINVAL, "overlap"),
            ("NULL", (p_in, 0, 0, R, q, ranks, 0, N), SA_EINVAL, "NULL"),
            ("q 9", (p_in, 0, p_out, R, 9, ranks + [0] * 6, 0, N), SA_EINVAL, "q must"),
            ("field 3", (p_in, 3, p_out, R, q, ranks, 0, N), SA_EINVAL, "field"),
            ("lo = hi", (p_in, 0, p_out, R, q, [0, 0, 0], 9, 9), SA_EINVAL, "range"),
            ("a rank at the width", (p_in, 0, p_out, R, q, [0, 100, 200], 50, 250), SA_EINVAL, "ranks[2] = 200"),
            ("a negative rank", (p_in, 0, p_out, R, q, [0, -1, 5], 0, N), SA_EINVAL, "ranks[1] = -1"),
            ("negative rows", (p_in, 0, p_out, -1, q, ranks, 0, N), SA_ESHAPE, "negative")):
        a_in, field, a_out, rows, qq, rk, lo, hi = args
        assert L.sa_rank_check(field, a_in, a_out, rows, qq, _c_ranks(rk), lo, hi) == code, tag
        assert L.sa_rank_f32(a_in, field, a_out, rows, qq, _c_ranks(rk), lo, hi, stream) == code, tag
        assert words in L.sa_rank_last_error().decode(), (tag, L.sa_rank_last_error())
    assert L.sa_rank_f32(p_in, 0, p_out, R, q, None, 0, N, stream) == SA_EINVAL and b"NULL ranks" in L.sa_rank_last_error()
    torch.cuda.synchronize()
    assert (out == 0xFF).all().item() and torch.equal(flat, before)
    assert L.sa_rank_f32(0, 0, 0, 0, q, _c_ranks(ranks), 0, N, stream) == SA_OK and L.sa_rank_last_error() == b""
    # `out` right behind `in`: touching is fine
    packed = torch.zeros((R * N * 4 + R * q * 4,), dtype=torch.uint8, device="cuda")
    packed[:R * N * 4] = x.view(torch.uint8).view(-1)
    base = packed.data_ptr()
    assert L.sa_rank_f32(base, 0, base + R * N * 4, R, q, _c_ranks(ranks), 0, N, stream) == SA_OK
    torch.cuda.synchronize()
    _same(packed[R * N * 4:].cpu().numpy().view(np.uint32).reshape(R, q), wide, ranks, "touching")
    # through the wrapper: shapes and dtypes before any device call
    for code, args, kw in ((SA_ESHAPE, (x[:, :N // 2], [0]), {}), (SA_EINVAL, (x.double(), [0]), {}),
                           (SA_ESHAPE, (x, [0]), dict(field="peak")),
                           (SA_ESHAPE, (x, [0, 1]), dict(out=torch.empty((R, 3), dtype=torch.float32, device="cuda"))),
                           (SA_ESHAPE, (x, [0, 1]), dict(out=torch.empty((R, 2), dtype=torch.int32, device="cuda"))),
                           (SA_ESHAPE, (x, [0, 1]), dict(out=torch.empty((R, 2), dtype=torch.float32))),
                           (SA_EINVAL, (x.cpu(), [0]), {})):
        with pytest.raises(SpecanError) as e:
            ch.order_stats(*args, **kw)
        assert e.value.code == code, (args[0].shape, kw)
    assert ch.order_stats(torch.empty((0, N), dtype=torch.float32, device="cuda"), [0, 5]).shape == (0, 2)
    mine = torch.zeros((R, 3), dtype=torch.float32, device="cuda")
    got = ch.order_stats(x, ranks, out=mine)
    assert got.data_ptr() == mine.data_ptr()
    _same(_bits(mine.cpu().numpy()), wide, ranks, "out=")


def test_poisoned_lds(ch, torch_mod, wide, lds_fill):
    """lds_fill(P) with P = 0xFFFFFFFF and 0x7F800000, then the call on the same stream: the bits of the mirror."""
    for field in FIELDS:
        x = to_device(torch_mod, _records(wide, field))
        for word in (0xFFFFFFFF, 0x7F800000):
            for ranks, lo, hi in (([8191], 0, N), (_rank_sets(N)[3], 0, N), ([0, 1, 2], 255, 1025)):
                lds_fill(word)
                got = _stats(ch, torch_mod, x, ranks, lo=lo, hi=hi, field=field)
                _same(got, wide, ranks, (field, hex(word), ranks), lo, hi)


@pytest.mark.parametrize("mode", [0xB1, 0xA1])
def test_the_top_rank_is_the_marker_of_the_float_chain(ch, torch_mod, mode):
    """Rank m - 1 over [lo, hi) is peak_mag of markers() with that marker range on the same frames, bit for bit -- float32,
    int16 and packed input; the full range and two ranges, one that holds the strongest tone and one that does not."""
    torch = torch_mod
    if mode == 0xA1:
        ch.load_sos(load_golden("g2_config1.npz")["sos"])
    ch.set_filter_mode(mode)
    for lo, hi in ((0, N), (1000, 1500), (2049, 5003)):
        ch.set_marker_range(lo, hi)
        assert ch.marker_range == (lo, hi)
        for form, x in _inputs(torch, _tones(4, 1820 + mode)).items():
            peak_mag, _, _ = ch.markers(x)
            top = ch.order_stats(ch.process_f32(x, out_kind="mag_full"), [hi - lo - 1], lo=lo, hi=hi)
            assert (peak_mag > 0).all().item(), form
            assert torch.equal(top[:, 0].view(torch.int32), peak_mag.view(torch.int32)), (form, lo, hi)


def test_the_top_rank_is_the_marker_of_the_integer_chain_and_the_peak_table(ch, torch_mod):
    torch = torch_mod
    x = to_device(torch, _tones(4, 1830))
    mag = ch.process_q15(x, out_kind="mag")
    for lo, hi in ((0, N), (2049, 5003)):
        ch.set_marker_range(lo, hi)
        peak_mag, _, _ = ch.markers_q15(x)
        top = ch.order_stats(mag, [hi - lo - 1], lo=lo, hi=hi)
        assert (peak_mag > 0).all().item()
        assert torch.equal(top[:, 0].view(torch.int32), peak_mag.view(torch.int32)), (lo, hi)
    # rank m - 1 over the full range is `mag` of find_peaks at K = 1, threshold 0
    peak, _, count = ch.find_peaks(mag, k=1)
    assert (count > 0).all().item()
    assert torch.equal(ch.order_stats(mag, [N - 1])[:, 0].view(torch.int32), peak[:, 0].contiguous().view(torch.int32))
    rec = ch.spectra_q15(x, 4)
    for field in ("peak", "power"):
        peak, _, _ = ch.find_peaks(rec, k=1, field=field)
        assert torch.equal(ch.order_stats(rec, [N - 1], field=field)[:, 0].view(torch.int32), peak[:, 0].contiguous().view(torch.int32))


def test_noise_floor_f32(ch, torch_mod):
    """int16 and packed frames, three tones and noise: the composed call equals the mirror on process_f32's magnitudes; with
    group = 4 the mirror on spectra_f32's power; the median lies far below the tones; the same with a caller's work and out,
    on a non-default stream and at overlap depth 2; a wrong work or out is refused before anything is launched."""
    from fpga_real_time_fft_analyzer_amd import frames
    from fpga_real_time_fft_analyzer_amd.abi import SpecanError
    torch = torch_mod
    ch.set_filter_mode(0xB1)
    B, qs, lo, hi = 4, [0.5, 0.1, 0.9, 1.0, 0.0], 100, 8000
    ranks = [frames.rank_of_quantile(v, hi - lo) for v in qs]
    assert ranks == [3949, 789, 7109, 7899, 0]                    # floor(q * 7899)
    forms = _inputs(torch, _tones(B, 1840))
    for form in ("int16", "uint8"):
        x = forms[form]
        m = ch.process_f32(x, out_kind="mag_full").cpu().numpy()
        want = _bits(frames.ranks_of_rows(m, ranks, lo, hi))
        got = ch.noise_floor_f32(x, qs, lo=lo, hi=hi)
        assert tuple(got.shape) == (B, 5) and np.array_equal(_bits(got.cpu().numpy()), want), form
        med = ch.noise_floor_f32(x)                               # the default: the lower median of the full range, [B, 1]
        assert tuple(med.shape) == (B, 1)
        assert np.array_equal(_bits(med.cpu().numpy()), _bits(frames.ranks_of_rows(m, [8191])))
        assert (med[:, 0] * 50 < torch.from_numpy(m).max(dim=1).values.cuda()).all().item()      # the floor is no tone
        rec = ch.spectra_f32(x, 4).cpu().numpy()
        want4 = _bits(frames.ranks_of_rows(rec, ranks, lo, hi, field="power"))
        got4 = ch.noise_floor_f32(x, qs, lo=lo, hi=hi, group=4)
        assert tuple(got4.shape) == (1, 5) and np.array_equal(_bits(got4.cpu().numpy()), want4), form
    x = forms["int16"]
    # a caller's work and out
    work = torch.full((B + 1, N), 3.0, dtype=torch.float32, device="cuda")
    out = torch.zeros((B, 5), dtype=torch.float32, device="cuda")
    m = ch.process_f32(x, out_kind="mag_full").cpu().numpy()
    want = _bits(frames.ranks_of_rows(m, ranks, lo, hi))
    res = ch.noise_floor_f32(x, qs, lo=lo, hi=hi, work=work, out=out)
    assert res.data_ptr() == out.data_ptr() and np.array_equal(_bits(out.cpu().numpy()), want)
    assert np.array_equal(work[:B].cpu().numpy(), m) and (work[B] == 3.0).all().item()
    # a non-default stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        res = ch.noise_floor_f32(x, qs, lo=lo, hi=hi, work=work)
    side.synchronize()
    assert np.array_equal(_bits(res.cpu().numpy()), want)
    # overlap depth 2: the input and the workspace dropped and scribbled over right behind the call
    want4 = _bits(frames.ranks_of_rows(ch.spectra_f32(x, 4).cpu().numpy(), ranks, lo, hi, field="power"))
    ch.set_overlap(2)
    for group, expect in ((None, want), (4, want4)):
        x2, w2 = x.clone(), torch.empty((B, N), dtype=torch.float32, device="cuda")
        res = ch.noise_floor_f32(x2, qs, lo=lo, hi=hi, group=group, work=w2)
        del x2, w2
        scribble = [torch.full((B, N), 7e7, dtype=torch.float32, device="cuda"), torch.full(x.shape, 85, dtype=x.dtype, device="cuda")]
        torch.cuda.synchronize()
        assert np.array_equal(_bits(res.cpu().numpy()), expect), group
        res = ch.noise_floor_f32(x, qs, lo=lo, hi=hi, group=group)     # and with the cached workspace
        torch.cuda.synchronize()
        assert np.array_equal(_bits(res.cpu().numpy()), expect), group
        del scribble
    ch.set_overlap(1)
    # refusals of the composed call, before any launch: the workspace and the out keep what they held
    for code, args, kw in ((SA_ESHAPE, (x[:3],), dict(group=4)), (SA_EINVAL, (x,), dict(group=3)), (SA_EINVAL, (x,), dict(q=1.5)),
                           (SA_EINVAL, (x,), dict(q=[0.5] * 9)), (SA_EINVAL, (x,), dict(lo=5, hi=5)),
                           (SA_ESHAPE, (x,), dict(work=torch.empty((B - 1, N), dtype=torch.float32, device="cuda"))),
                           (SA_ESHAPE, (x,), dict(work=torch.empty((B, N), dtype=torch.float64, device="cuda"))),
                           (SA_ESHAPE, (x,), dict(group=4, work=torch.empty((B - 1, N), dtype=torch.float32, device="cuda")))):
        out.fill_(-2.0)
        with pytest.raises(SpecanError) as e:
            ch.noise_floor_f32(*args, **dict(dict(q=qs, out=out if "group" not in kw else None), **kw))
        torch.cuda.synchronize()
        assert e.value.code == code and (out == -2.0).all().item(), kw
    for group, rows in ((None, B), (4, B // 4)):
        for bad in (torch.zeros((rows, 4), dtype=torch.float32, device="cuda"),
                    torch.zeros((rows + 1, 5), dtype=torch.float32, device="cuda"),
                    torch.zeros((rows, 5), dtype=torch.int32, device="cuda"), torch.zeros((rows, 5), dtype=torch.float32)):
            work.fill_(3.0)
            with pytest.raises(SpecanError) as e:
                ch.noise_floor_f32(x, qs, group=group, work=work, out=bad)
            torch.cuda.synchronize()
            assert e.value.code == SA_ESHAPE and (work == 3.0).all().item(), (group, bad.shape, bad.dtype)


def test_capture_and_replay(ch, torch_mod, wide):
    """order_stats captures without a warm-up -- it is one launch with its ranks in the launch's arguments -- and a replay
    after the input has changed gives the eager result of the new input; the host array of ranks is gone by then.  At depth 1,
    after one warm-up call of the same batch (it allocates the cached workspace), noise_floor_f32 captures too."""
    from fpga_real_time_fft_analyzer_amd import frames
    torch = torch_mod
    ranks = [8191, 0, N - 2, 100]
    x = to_device(torch, wide)
    out = torch.zeros((3, 4), dtype=torch.float32, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ch.order_stats(x, list(ranks), lo=1, hi=N, out=out)
    for pts in (wide[::-1] * np.float32(3.0), wide):
        pts = np.ascontiguousarray(pts)
        x.copy_(to_device(torch, pts))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        _same(_bits(out.cpu().numpy()), pts, ranks, "replay", 1, N)
    # the composed call
    ch.set_filter_mode(0xB1)
    assert ch.overlap == 1
    xs = [to_device(torch, _tones(4, 1850 + i, bins=(1000 + 700 * i, 3100, 6000 + 90 * i), amps=(900.0 / (1 + i), 450.0, 220.0)))
          for i in range(2)]
    eager = [_bits(ch.noise_floor_f32(xi, [0.5, 1.0]).cpu().numpy()) for xi in xs]
    assert not np.array_equal(eager[0], eager[1])
    xin = xs[0].clone()
    out2 = torch.zeros((4, 2), dtype=torch.float32, device="cuda")
    graph2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph2):
        ch.noise_floor_f32(xin, [0.5, 1.0], out=out2)
    for i in (1, 0):
        xin.copy_(xs[i])
        out2.zero_()
        graph2.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out2.cpu().numpy()), eager[i]), i
    assert "libspecan_rank.so" in open("/proc/self/maps").read()
