"""GPU: the peak table (include/specan_peaks.h: sa_peaks_f32 of libspecan_peaks.so), through SpectrumChain.find_peaks,
SpectrumChain.peak_table_f32 and the C entry point.

Every comparison is exact, on float bits and integers, records and counts, against the numpy mirror frames.peaks_of_rows,
whose probes tests/test_f32_peaks_cpu.py works out by hand; the probes are part of the data here, and their expected records
are asserted again on the device's.

The kernel's ownership (csrc/peaks_f32.hip): a row is dealt in 16-byte units, unit t + 256 j to thread t.  A unit is four
bins of magnitudes (field 0) or two bins of records (fields 1, 2), so a lane boundary lies at every multiple of 4 / 2 bins, a
wave boundary (64 lanes; the neighbour there comes from a load, not from the adjacent lane) at every multiple of 256 / 128
bins, and a thread's next unit starts 1024 / 512 bins further on; bins 0 and 16383 have a neighbour that does not exist.
EDGES holds the first and last bin on both sides of each kind of boundary for both unit sizes."""
import numpy as np
import pytest

from conftest import N, load_golden
from gpu_support import ch, lds_fill, to_device, torch_mod  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

SA_OK, SA_EINVAL, SA_ESHAPE = 0, -1, -2
FIELDS = (None, "peak", "power")
EDGES = (0, 1, 2, 3, 4, 5, 127, 128, 129, 255, 256, 257, 511, 512, 1023, 1024, 4095, 4096, 8191, 8192, 8193, 15359, 15360,
         16127, 16128, 16255, 16256, 16382, 16383)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _key(v):
    return int(_bits(np.float32(v)).ravel()[0]) & 0x7FFFFFFF


def _device_input(torch, pts, field):
    """``pts`` float32 [R, N] as the device tensor of the layout: itself, or records whose other float is a NaN"""
    if field is None:
        return to_device(torch, pts)
    rec = np.full(pts.shape + (2,), np.nan, np.float32)
    rec[..., 0 if field == "peak" else 1] = pts
    return to_device(torch, rec)


def _find(ch, torch, pts, field=None, **kw):
    """find_peaks on the device -> (mag bits uint32 [R,K], bin int32 [R,K], count int32 [R]) on the host"""
    mag, bins, count = ch.find_peaks(_device_input(torch, pts, field), field=field, **kw)
    torch.cuda.synchronize()
    return _bits(mag.contiguous().cpu().numpy()), bins.contiguous().cpu().numpy(), count.cpu().numpy()


def _same(got, pts, tag, **kw):
    """the device's records and counts against the mirror's, all bits"""
    from fpga_real_time_fft_analyzer_amd import frames
    mag, bins, count = frames.peaks_of_rows(pts, **kw)
    assert got[0].shape == mag.shape and got[1].dtype == np.int32 and got[2].dtype == np.int32, tag
    assert np.array_equal(got[2], count), (tag, "count", got[2], count)
    bad = np.nonzero(got[1] != bins)
    assert bad[0].size == 0, (tag, "bin", bad[0][:5], bad[1][:5], got[1][bad][:5], bins[bad][:5])
    bad = np.nonzero(got[0] != _bits(mag))
    assert bad[0].size == 0, (tag, "mag", bad[0][:5], bad[1][:5], got[0][bad][:5], _bits(mag)[bad][:5])
    return mag, bins, count


def _records(got, r=0):
    """row r as [(key, bin), ...] without the unused slots, which must be (+0.0, -1), and its count"""
    used = int((got[1][r] >= 0).sum())
    assert (got[1][r, used:] == -1).all() and not got[0][r, used:].any()
    return [(int(got[0][r, i]), int(got[1][r, i])) for i in range(used)], int(got[2][r])


@pytest.fixture(scope="module")
def wide():
    """R = 3 rows of exp(uniform +-60): about N / 3 candidates a row, count >> K"""
    rng = np.random.default_rng(1710)
    return np.exp(rng.uniform(-60.0, 60.0, size=(3, N))).astype(np.float32)


@pytest.mark.parametrize("field", FIELDS)
def test_every_k_and_min_sep_equals_the_mirror(ch, torch_mod, wide, field):
    x = _device_input(torch_mod, wide, field)
    for k in (1, 2, 7, 32):
        for min_sep in (1, 2, 5, 300, 16384):
            mag, bins, count = ch.find_peaks(x, k=k, min_sep=min_sep, field=field)
            got = (_bits(mag.contiguous().cpu().numpy()), bins.contiguous().cpu().numpy(), count.cpu().numpy())
            _, _, want = _same(got, wide, (field, k, min_sep), k=k, min_sep=min_sep)
            assert (want > 100 * 32).all()


@pytest.mark.parametrize("field", FIELDS)
def test_planted_peaks_and_plateaus_at_every_ownership_edge(ch, torch_mod, field):
    """On otherwise zero rows, at every bin b of EDGES: a lone peak at b, and across (b - 1, b) a rise (b is the peak), a fall
    (b - 1) and a two-bin plateau (b - 1, the lowest bin) -- the expected records by hand, and the mirror's."""
    rows, want = [], []
    for b in EDGES:
        patterns = [((b, 3.0),)] + ([((b - 1, 1.0), (b, 2.0)), ((b - 1, 2.0), (b, 1.0)), ((b - 1, 2.0), (b, 2.0))] if b else [])
        for i, pairs in enumerate(patterns):
            r = np.zeros(N, np.float32)
            for bin_, v in pairs:
                r[bin_] = v
            rows.append(r)
            want.append(([(_key(3.0), b)], [(_key(2.0), b)], [(_key(2.0), b - 1)], [(_key(2.0), b - 1)])[i])
    rows = np.stack(rows)
    for at in range(0, len(rows), 5):
        pts = rows[at:at + 5]
        got = _find(ch, torch_mod, pts, field, k=3)
        _same(got, pts, (field, at), k=3)
        for r in range(len(pts)):
            assert _records(got, r) == (want[at + r], 1), (field, at + r)
    # every edge bin a peak of its own value in one row (the neighbours among them excepted): all found, in order of value
    lone = [b for b in EDGES if b - 1 not in EDGES]
    pts = np.zeros((1, N), np.float32)
    for i, b in enumerate(lone):
        pts[0, b] = 1.0 + i
    got = _find(ch, torch_mod, pts, field, k=32)
    _same(got, pts, (field, "all edges"), k=32)
    assert _records(got) == ([(_key(1.0 + i), b) for i, b in reversed(list(enumerate(lone)))], len(lone))


def _row(pairs):
    r = np.zeros((1, N), np.float32)
    for b, v in pairs:
        r[0, b] = v
    return r


@pytest.mark.parametrize("field", FIELDS)
def test_hand_probes_on_the_device(ch, torch_mod, field):
    """The probes of tests/test_f32_peaks_cpu.py with their expected records, derived there."""
    k = _key
    probes = [
        (_row([(100, 5), (101, 5), (102, 5)]), dict(k=4), ([(k(5), 100)], 1)),
        (_row([(100, 5), (101, 5), (102, 7)]), dict(k=4), ([(k(7), 102), (k(5), 100)], 2)),
        (_row([(100, 5), (101, 5), (102, 7)]), dict(k=4, lo=101, hi=102), ([], 0)),
        (_row([(0, 2), (1, 2)]), dict(k=2), ([(k(2), 0)], 1)),
        (_row([(N - 2, 2), (N - 1, 2)]), dict(k=2), ([(k(2), N - 2)], 1)),
        (_row([(0, 2), (N - 1, 3)]), dict(k=2), ([(k(3), N - 1), (k(2), 0)], 2)),
        (_row([(50, 4), (51, 6), (60, 6), (61, 4), (70, 7), (71, 7)]), dict(k=8), ([(k(7), 70), (k(6), 51), (k(6), 60)], 3)),
        (_row([(900, 3), (300, 3), (600, 3), (100, 1), (1200, 8)]), dict(k=3), ([(k(8), 1200), (k(3), 300), (k(3), 600)], 5)),
        (_row([(40, 2.5), (80, 9)]), dict(k=4, threshold=2.5), ([(k(9), 80), (k(2.5), 40)], 2)),
        (_row([(40, 2.5), (80, 9)]), dict(k=4, threshold=float(np.nextafter(np.float32(2.5), np.float32(3)))), ([(k(9), 80)], 1)),
        (_row([(40, 2.5), (80, 9)]), dict(k=4, threshold=10.0), ([], 0)),                  # above the row's maximum
        (_row([(499, 7), (500, 5)]), dict(k=4, lo=500, hi=600), ([], 0)),
        (_row([(500, 5), (501, 5)]), dict(k=4, lo=400, hi=501), ([(k(5), 500)], 1)),
        (_row([(98, 9), (100, 5)]), dict(k=4, lo=100, hi=200, min_sep=50), ([(k(5), 100)], 1)),
        (_row([(100, 10), (103, 9), (106, 8)]), dict(k=8, min_sep=4), ([(k(10), 100), (k(8), 106)], 3)),
        (_row([(100, 10), (103, 9), (106, 8)]), dict(k=8, min_sep=3), ([(k(10), 100), (k(9), 103), (k(8), 106)], 3)),
        (_row([(100, 4), (106, 4), (113, 4)]), dict(k=8, min_sep=7), ([(k(4), 100), (k(4), 113)], 3)),
        (_row([(0, 3), (N - 1, 3)]), dict(k=8, min_sep=N), ([(k(3), 0)], 2)),
        (_row([(0, 3), (N - 1, 3)]), dict(k=8, min_sep=N - 1), ([(k(3), 0), (k(3), N - 1)], 2)),
        (_row([(10, 3e38), (20, np.inf), (30, np.nan), (40, -np.inf), (50, -7.0)]), dict(k=8),
         ([(0x7FC00000, 30), (0x7F800000, 20), (0x7F800000, 40), (k(3e38), 10), (k(7.0), 50)], 5)),
        (_row([(5, -0.0), (6, -0.0)]), dict(k=2), ([], 0)),
        (_row([(60, 2.0 ** -149), (70, 2.0 ** -140), (80, -(2.0 ** -130))]), dict(k=4), ([(1 << 19, 80), (0x200, 70), (1, 60)], 3)),
        (_row([(60, 2.0 ** -149), (70, 2.0 ** -140)]), dict(k=4, threshold=2.0 ** -140), ([(0x200, 70)], 1)),
        (_row([(90, -3.0), (91, 2.0)]), dict(k=4), ([(k(3.0), 90)], 1)),
        (np.zeros((1, N), np.float32), dict(k=5), ([], 0)),
    ]
    for i, (pts, kw, want) in enumerate(probes):
        got = _find(ch, torch_mod, pts, field, **kw)
        assert _records(got) == want, (field, i, kw)
        _same(got, pts, (field, i), **kw)
    pts = np.zeros((1, N), np.float32)
    pts.view(np.uint32)[0, 77] = 0xFFC00123                       # a negative NaN: the sign cleared, the payload kept
    assert _records(_find(ch, torch_mod, pts, field, k=2)) == ([(0x7FC00123, 77)], 1)


@pytest.mark.parametrize("field", FIELDS)
def test_ranges_thresholds_and_ties(ch, torch_mod, wide, field):
    x = _device_input(torch_mod, wide, field)

    def run(pts, dev, **kw):
        mag, bins, count = ch.find_peaks(dev, field=field, **kw)
        got = (_bits(mag.contiguous().cpu().numpy()), bins.contiguous().cpu().numpy(), count.cpu().numpy())
        return got, _same(got, pts, (field, kw), **kw)

    # lo and hi on and off the unit, wave and round boundaries
    for lo, hi in ((0, 1), (N - 1, N), (1, N - 1), (256, 512), (255, 513), (257, 511), (1024, 2048), (1021, 2051), (4096, 4100),
                   (4097, 4099), (8191, 8193), (127, 129), (5000, 5001), (3, 16381)):
        run(wide, x, k=7, lo=lo, hi=hi, min_sep=3)
    # thresholds: one that leaves a handful, and one above the maximum of every row
    top = np.sort(wide, axis=1)[:, -5].min()
    got, (_, _, count) = run(wide, x, k=32, threshold=float(top))
    assert (count >= 1).all() and (count <= (wide >= top).sum(axis=1)).all() and (count < 32).all()     # the maximum is one
    got, _ = run(wide, x, k=4, threshold=float(np.float32(wide.max()) * np.float32(2.0)))
    assert not got[2].any() and (got[1] == -1).all() and not got[0].any()
    # a mirrored row, row[k] == row[N - k]: every tie goes to the lower bin
    m = wide.copy()
    m[:, N // 2 + 1:] = m[:, 1:N // 2][:, ::-1]
    assert np.array_equal(m[:, 1:], m[:, 1:][:, ::-1])
    got, _ = run(m, _device_input(torch_mod, m, field), k=32, min_sep=2)
    pairs = got[1][:, 0::2], got[1][:, 1::2]
    paired = pairs[0] + pairs[1] == N
    assert paired.mean() > 0.8 and (pairs[0][paired] < pairs[1][paired]).all()
    # equal peaks owned by different waves and threads: the same value at one bin of every wave of every round
    e = np.zeros((1, N), np.float32)
    where = [64 * 4 * w + 1024 * j + 4 * (5 * w + j) + (w + j) % 4 for j in range(8) for w in range(4)]
    e[0, where] = 6.0
    got, _ = run(e, _device_input(torch_mod, e, field), k=32)
    assert _records(got) == ([(_key(6.0), b) for b in sorted(where)], 32)
    got, _ = run(e, _device_input(torch_mod, e, field), k=5, min_sep=300)
    assert [b for _, b in _records(got)[0]] == [sorted(where)[i] for i in (0, 2, 4, 6, 8)]       # 266 or 278 apart: every second


def test_specials_in_wide_rows(ch, torch_mod, wide):
    """R = 5 with row 2 all NaN and row 3 all +inf: rows 0, 1 and 4 equal their single-row calls, and the two special rows
    have one candidate each, bin 0 (a plateau over the whole row)."""
    pts = np.concatenate([wide[:2], np.full((1, N), np.nan, np.float32), np.full((1, N), np.inf, np.float32), wide[2:]])
    pts[0, 4000] = np.nan
    pts[0, 9000] = -np.inf
    pts[1, 12000] = -0.0
    pts[4, 0] = np.inf
    for field in FIELDS:
        got = _find(ch, torch_mod, pts, field, k=7, min_sep=2)
        _same(got, pts, field, k=7, min_sep=2)
        assert _records(got, 2) == ([(0x7FC00000, 0)], 1) and _records(got, 3) == ([(0x7F800000, 0)], 1)
        assert (got[0][0, 0], got[1][0, 0]) == (0x7FC00000, 4000) and (got[0][0, 1], got[1][0, 1]) == (0x7F800000, 9000)
        for r in (0, 1, 4):
            one = _find(ch, torch_mod, pts[r:r + 1], field, k=7, min_sep=2)
            for a, b in zip(got, one):
                assert np.array_equal(a[r:r + 1], b), (field, r)


def test_exactly_the_output_bytes_are_written_and_a_refused_call_writes_nothing(ch, torch_mod, wide):
    from fpga_real_time_fft_analyzer_amd import abi, frames
    torch = torch_mod
    L = abi.peaks_lib()
    stream = torch.cuda.current_stream().cuda_stream
    R, K, guard = 3, 7, 4096
    x = to_device(torch, wide)
    out = torch.full((R * K * 8 + guard,), 0xFF, dtype=torch.uint8, device="cuda")
    count = torch.full((R * 4 + guard,), 0xFF, dtype=torch.uint8, device="cuda")
    assert L.sa_peaks_f32(x.data_ptr(), 0, out.data_ptr(), count.data_ptr(), R, K, 0.0, 0, N, 1, stream) == SA_OK
    assert L.sa_peaks_last_error() == b""
    torch.cuda.synchronize()
    assert (out[R * K * 8:] == 0xFF).all().item() and (count[R * 4:] == 0xFF).all().item()
    rec = out[:R * K * 8].cpu().numpy().view(np.uint32).reshape(R, K, 2)
    cnt = count[:R * 4].cpu().numpy().view(np.int32)
    assert (rec != 0xFFFFFFFF).all() and (cnt != -1).all()                   # every word of both was written
    _same((rec[..., 0], rec[..., 1].view(np.int32), cnt), wide, "C call", k=K)
    # an all-zero row: the unused slots are written too, (+0.0, -1)
    z = torch.zeros((1, N), dtype=torch.float32, device="cuda")
    out.fill_(0xFF)
    count.fill_(0xFF)
    assert L.sa_peaks_f32(z.data_ptr(), 0, out.data_ptr(), count.data_ptr(), 1, K, 0.0, 0, N, 1, stream) == SA_OK
    torch.cuda.synchronize()
    rec = out[:K * 8].cpu().numpy().view(np.uint32).reshape(K, 2)
    assert not rec[:, 0].any() and (rec[:, 1] == 0xFFFFFFFF).all() and count[:4].cpu().numpy().view(np.int32)[0] == 0
    assert (out[K * 8:] == 0xFF).all().item() and (count[4:] == 0xFF).all().item()
    # refused calls: the code of sa_peaks_check for the same integers, its text, and nothing written
    out.fill_(0xFF)
    count.fill_(0xFF)
    flat = torch.zeros((R * N + 64,), dtype=torch.float32, device="cuda")
    before = flat.clone()
    nan_bits, cases = 0x7FC00000, []
    p_in, p_out, p_count = flat.data_ptr(), out.data_ptr(), count.data_ptr()
    for tag, args, code, words in (
            ("in 4 bytes off", (p_in + 4, 0, p_out, p_count, R, K, 0, 0, N, 1), SA_EINVAL, "`in` must be 16-byte aligned"),
            ("out 4 bytes off", (p_in, 0, p_out + 4, p_count, R, K, 0, 0, N, 1), SA_EINVAL, "`out` must be 8-byte aligned"),
            ("count 2 bytes off", (p_in, 0, p_out, p_count + 2, R, K, 0, 0, N, 1), SA_EINVAL, "`count` must be 4-byte aligned"),
            ("out inside in", (p_in, 0, p_in + R * N * 4 - 8, p_count, R, K, 0, 0, N, 1), SA_EINVAL, "overlap"),
            ("count inside out", (p_in, 0, p_out, p_out + 8, R, K, 0, 0, N, 1), SA_EINVAL, "overlap"),
            ("records read twice as much", (p_in, 2, p_in + R * N * 4, p_count, R, K, 0, 0, N, 1), SA_EINVAL, "overlap"),
            ("NULL", (p_in, 0, 0, p_count, R, K, 0, 0, N, 1), SA_EINVAL, "NULL"),
            ("k 33", (p_in, 0, p_out, p_count, R, 33, 0, 0, N, 1), SA_EINVAL, "k must"),
            ("field 3", (p_in, 3, p_out, p_count, R, K, 0, 0, N, 1), SA_EINVAL, "field"),
            ("a NaN threshold", (p_in, 0, p_out, p_count, R, K, nan_bits, 0, N, 1), SA_EINVAL, "threshold"),
            ("a negative threshold", (p_in, 0, p_out, p_count, R, K, 0xBF800000, 0, N, 1), SA_EINVAL, "threshold"),
            ("lo = hi", (p_in, 0, p_out, p_count, R, K, 0, 9, 9, 1), SA_EINVAL, "range"),
            ("min_sep 0", (p_in, 0, p_out, p_count, R, K, 0, 0, N, 0), SA_EINVAL, "min_sep"),
            ("negative rows", (p_in, 0, p_out, p_count, -1, K, 0, 0, N, 1), SA_ESHAPE, "negative")):
        a_in, field, a_out, a_count, rows, k, thr, lo, hi, sep = args
        assert L.sa_peaks_check(field, a_in, a_out, a_count, rows, k, thr, lo, hi, sep) == code, tag
        threshold = float(np.array([thr], np.uint32).view(np.float32)[0])
        assert L.sa_peaks_f32(a_in, field, a_out, a_count, rows, k, threshold, lo, hi, sep, stream) == code, tag
        assert words in L.sa_peaks_last_error().decode(), (tag, L.sa_peaks_last_error())
    torch.cuda.synchronize()
    assert (out == 0xFF).all().item() and (count == 0xFF).all().item() and torch.equal(flat, before)
    assert L.sa_peaks_f32(0, 0, 0, 0, 0, K, 0.0, 0, N, 1, stream) == SA_OK and L.sa_peaks_last_error() == b""
    # `out` right behind `in` and `count` right behind `out`: touching is fine
    packed = torch.zeros((R * N * 4 + R * K * 8 + R * 4,), dtype=torch.uint8, device="cuda")
    packed[:R * N * 4] = x.view(torch.uint8).view(-1)
    base = packed.data_ptr()
    assert L.sa_peaks_f32(base, 0, base + R * N * 4, base + R * N * 4 + R * K * 8, R, K, 0.0, 0, N, 1, stream) == SA_OK
    torch.cuda.synchronize()
    tail = packed[R * N * 4:].cpu().numpy()
    rec = tail[:R * K * 8].view(np.uint32).reshape(R, K, 2)
    _same((rec[..., 0], rec[..., 1].view(np.int32), tail[R * K * 8:].view(np.int32)), wide, "touching", k=K)
    # through the wrapper: shapes and dtypes before any device call
    from fpga_real_time_fft_analyzer_amd.abi import SpecanError
    for code, args, kw in ((SA_ESHAPE, (x[:, :N // 2],), {}), (SA_EINVAL, (x.double(),), {}), (SA_ESHAPE, (x,), dict(field="peak")),
                           (SA_ESHAPE, (x,), dict(k=4, out=torch.empty((R, 5, 2), dtype=torch.int32, device="cuda"))),
                           (SA_ESHAPE, (x,), dict(k=4, out=torch.empty((R, 4, 2), dtype=torch.float32, device="cuda"))),
                           (SA_EINVAL, (x.cpu(),), {})):
        with pytest.raises(SpecanError) as e:
            ch.find_peaks(*args, **kw)
        assert e.value.code == code, (args[0].shape, kw)
    mag, bins, cnt = ch.find_peaks(torch.empty((0, N), dtype=torch.float32, device="cuda"), k=4)
    assert mag.shape == (0, 4) and bins.shape == (0, 4) and cnt.shape == (0,)
    mine = torch.zeros((R, K, 2), dtype=torch.int32, device="cuda")
    mag, bins, cnt = ch.find_peaks(x, k=K, out=mine)
    assert mag.data_ptr() == mine.data_ptr() and bins.data_ptr() == mine.data_ptr() + 4
    want = frames.peaks_of_rows(wide, K)
    assert np.array_equal(mine.cpu().numpy()[..., 1], want[1]) and np.array_equal(_bits(mag.contiguous().cpu().numpy()), _bits(want[0]))


def test_poisoned_lds(ch, torch_mod, wide, lds_fill):
    """lds_fill(P) with P = 0xFFFFFFFF and 0x7F800000, then the call on the same stream: the bits of the mirror."""
    for field in FIELDS:
        x = _device_input(torch_mod, wide, field)
        for word in (0xFFFFFFFF, 0x7F800000):
            for kw in (dict(k=32, min_sep=5), dict(k=1), dict(k=4, threshold=1e30)):
                lds_fill(word)
                mag, bins, count = ch.find_peaks(x, field=field, **kw)
                got = (_bits(mag.contiguous().cpu().numpy()), bins.contiguous().cpu().numpy(), count.cpu().numpy())
                _same(got, wide, (field, hex(word), kw), **kw)


def _inputs(torch, xi):
    """the three input forms of one batch of 12-bit samples: float32 (sample / 2048), int16, packed uint8"""
    from fpga_real_time_fft_analyzer_amd.ingest import pack12
    return {"float32": to_device(torch, (xi / 2048.0).astype(np.float32)), "int16": to_device(torch, xi),
            "uint8": to_device(torch, pack12(xi))}


def _tones(B, seed, bins=(1200, 3000, 5500), amps=(900.0, 450.0, 220.0)):
    """int16 [B, N]: three tones on whole bins, of falling amplitude, plus noise"""
    rng = np.random.default_rng(seed)
    n = np.arange(N)
    x = sum(a * np.sin(2 * np.pi * b * n / N + rng.uniform(0, 2 * np.pi, (B, 1))) for a, b in zip(amps, bins))
    return np.clip(np.rint(x + 20.0 * rng.standard_normal((B, N))), -2048, 2047).astype(np.int16)


@pytest.mark.parametrize("mode", [0xB1, 0xA1])
def test_k1_is_the_marker_of_the_float_chain(ch, torch_mod, mode):
    """K = 1, threshold 0, the range (0, 16384): (mag, bin) is (peak_mag, peak_bin) of markers() on the same frames, bit for
    bit -- float32, int16 and packed input."""
    torch = torch_mod
    if mode == 0xA1:
        ch.load_sos(load_golden("g2_config1.npz")["sos"])
    ch.set_filter_mode(mode)
    assert ch.marker_range == (0, N)
    for form, x in _inputs(torch, _tones(4, 1720 + mode)).items():
        peak_mag, peak_bin, _ = ch.markers(x)
        mag, bins, count = ch.find_peaks(ch.process_f32(x, out_kind="mag_full"), k=1)
        assert (peak_mag > 0).all().item() and (count > 0).all().item(), form
        assert torch.equal(bins[:, 0], peak_bin) and torch.equal(mag[:, 0].view(torch.int32), peak_mag.view(torch.int32)), form


def test_k1_is_the_marker_of_the_integer_chain(ch, torch_mod):
    torch = torch_mod
    x = to_device(torch, _tones(4, 1730))
    peak_mag, peak_bin, _ = ch.markers_q15(x)
    mag, bins, count = ch.find_peaks(ch.process_q15(x, out_kind="mag"), k=1)
    assert (peak_mag > 0).all().item() and (count > 0).all().item()
    assert torch.equal(bins[:, 0], peak_bin) and torch.equal(mag[:, 0].view(torch.int32), peak_mag.view(torch.int32))
    # and behind the integer fold: the max hold of spectra_q15 is a record layout
    rec = ch.spectra_q15(x, 4)
    mag, bins, _ = ch.find_peaks(rec, k=1, field="peak")
    hold = rec[..., 0].contiguous()
    assert torch.equal(bins[:, 0].long(), hold.argmax(dim=1)) and torch.equal(mag[:, 0], hold.max(dim=1).values)


def _host(t3):
    return tuple(np.ascontiguousarray(t.contiguous().cpu().numpy()).view(np.uint32) for t in t3)


def test_peak_table_f32(ch, torch_mod):
    """int16 frames, three tones on whole bins and noise: the composed call equals find_peaks(process_f32(...)); with group = 4
    find_peaks(spectra_f32(...), field='power'); the three tones and their mirrors are the first six bins found; the same on
    a non-default stream, with a caller's work and out, at overlap depth 2, and captured into a graph and replayed."""
    from fpga_real_time_fft_analyzer_amd import frames
    torch = torch_mod
    ch.set_filter_mode(0xB1)
    B, kw = 4, dict(k=8, min_sep=16, threshold=1e-3)
    xi = _tones(B, 1740)
    x = to_device(torch, xi)
    mag_full = ch.process_f32(x, out_kind="mag_full")
    want = _host(ch.find_peaks(mag_full, **kw))
    m = mag_full.cpu().numpy()
    ref = frames.peaks_of_rows(m, **kw)
    assert all(np.array_equal(w, np.ascontiguousarray(r).view(np.uint32)) for w, r in zip(want, ref))
    got = _host(ch.peak_table_f32(x, **kw))
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    tones = [1200, N - 1200, 3000, N - 3000, 5500, N - 5500]
    assert (want[1].view(np.int32)[:, :6] == np.array(tones)).all(), want[1].view(np.int32)[:, :6]
    # group = 4: the peaks of the Welch sum
    rec = ch.spectra_f32(x, 4)
    want4 = _host(ch.find_peaks(rec, field="power", **kw))
    ref4 = frames.peaks_of_rows(np.ascontiguousarray(rec.cpu().numpy()[..., 1]), **kw)
    assert all(np.array_equal(w, np.ascontiguousarray(r).view(np.uint32)) for w, r in zip(want4, ref4))
    got4 = _host(ch.peak_table_f32(x, group=4, **kw))
    assert all(np.array_equal(g, w) for g, w in zip(got4, want4))
    assert got4[0].shape == (1, 8) and (got4[1].view(np.int32)[0, :6] == np.array(tones)).all()
    # a caller's work and out
    work = torch.full((B + 1, N), 3.0, dtype=torch.float32, device="cuda")
    out = torch.zeros((B, 8, 2), dtype=torch.int32, device="cuda")
    res = ch.peak_table_f32(x, work=work, out=out, **kw)
    assert res[0].data_ptr() == out.data_ptr() and all(np.array_equal(g, w) for g, w in zip(_host(res), want))
    assert np.array_equal(work[:B].cpu().numpy(), m) and (work[B] == 3.0).all().item()
    # a non-default stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        res = ch.peak_table_f32(x, work=work, **kw)
        res4 = ch.find_peaks(rec, field="power", **kw)
    side.synchronize()
    assert all(np.array_equal(g, w) for g, w in zip(_host(res), want))
    assert all(np.array_equal(g, w) for g, w in zip(_host(res4), want4))
    # overlap depth 2: the input and the workspace dropped and scribbled over right behind the call
    ch.set_overlap(2)
    for group, expect in ((None, want), (4, want4)):
        x2, w2 = x.clone(), torch.empty((B, N), dtype=torch.float32, device="cuda")
        res = ch.peak_table_f32(x2, group=group, work=w2, **kw)
        del x2, w2
        scribble = [torch.full((B, N), 7e7, dtype=torch.float32, device="cuda"), torch.full(x.shape, 85, dtype=x.dtype, device="cuda")]
        torch.cuda.synchronize()
        assert all(np.array_equal(g, w) for g, w in zip(_host(res), expect)), group
        res = ch.peak_table_f32(x, group=group, **kw)             # and with the cached workspace
        torch.cuda.synchronize()
        assert all(np.array_equal(g, w) for g, w in zip(_host(res), expect)), group
        del scribble
    ch.set_overlap(1)
    # refusals of the composed call, before any launch
    from fpga_real_time_fft_analyzer_amd.abi import SpecanError
    for code, args, kw2 in ((SA_ESHAPE, (x[:3],), dict(group=4)), (SA_EINVAL, (x,), dict(group=3)), (SA_EINVAL, (x,), dict(k=0)),
                            (SA_ESHAPE, (x,), dict(work=torch.empty((B - 1, N), dtype=torch.float32, device="cuda")))):
        with pytest.raises(SpecanError) as e:
            ch.peak_table_f32(*args, **kw2)
        assert e.value.code == code, kw2
    # a wrong `out` is refused before the chain is launched: the caller's workspace keeps what it held
    for group, rows in ((None, B), (4, B // 4)):
        for bad in (torch.zeros((rows, 7, 2), dtype=torch.int32, device="cuda"), torch.zeros((rows + 1, 8, 2), dtype=torch.int32, device="cuda"),
                    torch.zeros((rows, 8, 2), dtype=torch.float32, device="cuda"), torch.zeros((rows, 8, 2), dtype=torch.int32)):
            work.fill_(3.0)
            with pytest.raises(SpecanError) as e:
                ch.peak_table_f32(x, group=group, work=work, out=bad, **kw)
            torch.cuda.synchronize()
            assert e.value.code == SA_ESHAPE and (work == 3.0).all().item(), (group, bad.shape, bad.dtype)


def test_capture_and_replay(ch, torch_mod):
    """Depth 1: after one warm-up call of the same batch (it allocates the cached workspace) peak_table_f32 is captured and
    replayed on new input: the eager result of that input, bit for bit.  The find alone captures without a warm-up."""
    torch = torch_mod
    ch.set_filter_mode(0xB1)
    B, kw = 4, dict(k=8, min_sep=16)
    assert ch.overlap == 1
    xs = [to_device(torch, _tones(B, 1750 + i, bins=(1000 + 700 * i, 3100, 6000 + 90 * i))) for i in range(2)]
    eager = [_host(ch.peak_table_f32(xi, **kw)) for xi in xs]
    assert not np.array_equal(eager[0][1], eager[1][1])
    x = xs[0].clone()
    out = torch.zeros((B, 8, 2), dtype=torch.int32, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = ch.peak_table_f32(x, out=out, **kw)
    for i in (1, 0):
        x.copy_(xs[i])
        out.zero_()
        res[2].zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(np.array_equal(g, w) for g, w in zip(_host(res), eager[i])), i
    mag = ch.process_f32(xs[1], out_kind="mag_full")
    out2 = torch.zeros_like(out)
    graph2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph2):
        res2 = ch.find_peaks(mag, out=out2, **kw)
    graph2.replay()
    torch.cuda.synchronize()
    assert all(np.array_equal(g, w) for g, w in zip(_host(res2), eager[1]))
    assert "libspecan_peaks.so" in open("/proc/self/maps").read()
