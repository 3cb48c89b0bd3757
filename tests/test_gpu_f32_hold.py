"""GPU: the percentile traces (include/specan_hold.h: sa_hold_f32 of libspecan_hold.so), through SpectrumChain.hold_ranks,
SpectrumChain.hold_f32 and the C entry point.

Every comparison is exact, on float bits, against the numpy mirror frames.holds_of_rows, whose probes
tests/test_f32_hold_cpu.py works out by hand; the probes are planted here at the kernel's ownership boundaries and their
expected bits asserted again on the device's.  torch.sort of the keys, the float fold and torch.amin are references that share
nothing with the mirror.

The kernel's ownership (csrc/hold_f32.hip, csrc/sa_hold.hpp): a group of A rows is served by the register class AMAX = 8, 16,
32, 64 or 128, the smallest that holds A.  Thread t of workgroup y (256 threads; the groups are on the grid's x) owns the
BINS adjacent bins from BINS (256 y + t) on: BINS = 4 (magnitudes) or 2 (records) in the classes 8 and 16, one 16-byte load
per row, and BINS = 1 in the classes 32 to 128, one 4-byte load per row.  So a thread's bins end at every multiple of BINS,
a wave's at every multiple of 64 BINS and a workgroup's at every multiple of 256 BINS: edges(BINS) is the first and the last
bin on both sides of the first and the last of each of these boundaries, and of the row's ends."""
import ctypes

import numpy as np
import pytest

from conftest import N
from gpu_support import ch, check_overlap_profiling_and_graph_capture, to_device, torch_mod  # noqa: F401 (fixtures)
from reduction_libraries import FIELDS, SA_EINVAL, SA_ESHAPE, SA_OK, bits, key, records_of
from test_f32_hold_cpu import CLASSES, ONE, ONE_UP, SPECIALS, SPECIALS_SORTED, hold_bins, hold_class
from test_gpu_f32_peaks import _inputs, _tones

pytestmark = pytest.mark.gpu

G = 3
# the lowest and the highest group of every class -- one on either side of each class boundary -- and the odd sizes
GROUPS = (2, 3, 5, 7, 8, 9, 16, 17, 32, 33, 64, 65, 127, 128)
assert {hold_class(a) for a in GROUPS} == set(CLASSES) and all(c in GROUPS and c + 1 in GROUPS for c in CLASSES[:-1])


def edges(bins_per_thread):
    """the first and last bin on both sides of the first and last thread, wave and workgroup boundary (module docstring)"""
    out = {0, N - 1}
    for step in (bins_per_thread, 64 * bins_per_thread, 256 * bins_per_thread):
        for at in (step, N - step):
            out |= {at - 1, at}
    return sorted(out)


def rank_sets(A):
    """the rank sets of a group of A: the min hold, the max hold, five across, and eight unsorted with repeats"""
    five = [0, min(1, A - 1), A // 2, max(A - 2, 0), A - 1]
    eight = [A - 1, 0, A // 3, A - 1, (2 * A) // 3, A // 3, min(7, A - 1), A // 2]
    return [0], [A - 1], five, eight


@pytest.fixture(scope="module")
def wide():
    """4 * 128 rows of exp(uniform +-60): keys spread over 170 exponents, every bit of a key in play and all keys distinct, so
    that a point read from the wrong row or bin shows"""
    rng = np.random.default_rng(2710)
    a = np.exp(rng.uniform(-60.0, 60.0, size=(4 * 128, N))).astype(np.float32)
    a.setflags(write=False)
    return a


def _traces(ch, torch, x, ranks, A, **kw):
    """hold_ranks on the device tensor -> its bits uint32 [G, q, N] on the host"""
    got = ch.hold_ranks(x, ranks, A, **kw)
    assert got.dtype == torch.float32 and tuple(got.shape) == (x.shape[0] // A, len(ranks), N) and got.is_contiguous()
    return bits(got.cpu().numpy())


def _same(got, pts, ranks, A, tag):
    """the device's bits against the mirror's on the plain points"""
    from fpga_real_time_fft_analyzer_amd import frames
    want = bits(frames.holds_of_rows(pts, ranks, A))
    bad = np.nonzero(got != want)
    assert got.shape == want.shape and bad[0].size == 0, (tag, [b[:5] for b in bad], got[bad][:5], want[bad][:5])
    return want


_mirrored = {}                  # (A, ranks) -> the mirror's bits on the first G * A rows of `wide`, computed once


@pytest.mark.parametrize("field", FIELDS)
def test_every_class_and_rank_set_equals_the_mirror(ch, torch_mod, wide, field):
    """G = 3 groups of every A of GROUPS: the group's stride and index matter, and every class is entered at its lowest and
    highest A."""
    x = to_device(torch_mod, records_of(wide, field))
    for A in GROUPS:
        low, high, five, eight = rank_sets(A)
        for ranks in (five, eight):
            if (A, tuple(ranks)) not in _mirrored:                # the three fields hold the same points: one mirror for all
                _mirrored[A, tuple(ranks)] = _same(_traces(ch, torch_mod, x[:G * A], ranks, A, field=field), wide[:G * A], ranks,
                                                   A, (field, A, ranks))
        across = _mirrored[A, tuple(five)]                        # the two holds are the ends of the five
        for ranks, want in ((five, across), (eight, _mirrored[A, tuple(eight)]), (low, across[:, :1]), (high, across[:, 4:])):
            got = _traces(ch, torch_mod, x[:G * A], ranks, A, field=field)
            assert np.array_equal(got, want), (field, A, ranks, np.nonzero(got != want)[0][:5])


@pytest.mark.parametrize("field", FIELDS)
def test_hand_probes_at_the_ownership_boundaries(ch, torch_mod, field):
    """The probes of tests/test_f32_hold_cpu.py with their expected bits, derived there, planted at every bin of edges(BINS)
    for the load width of the class: A = 5 (class 8: 16-byte loads, BINS = 4 or 2) and A = 33 (class 64: BINS = 1), two
    groups each.  The last-bit probe: rows of 1.0, and at edge bin k one row (k mod A, so every row takes its turn) is one ulp
    up: the max hold alone shows it, at that bin alone.  The specials: six frames of an edge bin hold NaN, +inf, -3.0, 2.0,
    the denormal of bits 1 and -0.0; their sorted keys are the six traces there, and zero elsewhere."""
    torch = torch_mod
    up = np.nextafter(np.float32(1), np.float32(2), dtype=np.float32)
    for A in (5, 33):
        at = edges(hold_bins(hold_class(A), field))
        pts = np.ones((2 * A, N), np.float32)
        for k, b in enumerate(at):
            pts[A + k % A, b] = up                                # in the second group: its row offset matters
        got = _traces(ch, torch, to_device(torch, records_of(pts, field)), [A - 1, A - 2, 0], A, field=field)
        want = np.full((2, 3, N), ONE, np.uint32)
        want[1, 0, at] = ONE_UP
        assert np.array_equal(got, want), (field, A, np.nonzero(got != want))
        _same(got, pts, [A - 1, A - 2, 0], A, (field, A, "last bit"))
    for A in (6, 40):                                             # six specials, and 34 zeros below them
        at = edges(hold_bins(hold_class(A), field))
        pts = np.zeros((2 * A, N), np.float32)
        for k, b in enumerate(at):
            rows = (np.arange(6) * 5 + k) % A                     # six different rows of the group, others per edge
            assert len(set(rows)) == 6
            pts[rows, b] = np.array(SPECIALS, np.float32)
        ranks = list(range(A - 6, A))
        got = _traces(ch, torch, to_device(torch, records_of(pts, field)), ranks, A, field=field)
        want = np.zeros((2, 6, N), np.uint32)
        want[0][:, at] = np.array(SPECIALS_SORTED, np.uint32)[:, None]
        assert np.array_equal(got, want), (field, A)
        _same(got, pts, ranks, A, (field, A, "specials"))
        if A > 6:                                                 # the zeros below the six
            assert not _traces(ch, torch, to_device(torch, records_of(pts, field)), [0, A - 7], A, field=field).any()
    # ties that straddle a rank, and repeated and unsorted ranks on the ramp of the CPU file
    pts = np.zeros((7, N), np.float32)
    pts[:, 100] = (5, 9, 5, 2, 5, 9, 5)
    got = _traces(ch, torch, to_device(torch, records_of(pts, field)), [0, 1, 3, 4, 5, 6], 7, field=field)
    assert got[0, :, 100].tolist() == [key(v) for v in (2, 5, 5, 5, 9, 9)] and not got[0, :, :100].any()
    A = 15
    ramp = (np.arange(A, dtype=np.float32)[:, None] + np.arange(N, dtype=np.float32)[None, :] / N).astype(np.float32)
    ranks = [9, 3, 9, A - 1, 0, 3, 7, 9]
    got = _traces(ch, torch, to_device(torch, records_of(ramp[::-1], field)), ranks, A, field=field)
    want = bits((np.array(ranks, np.float32)[:, None] + np.arange(N, dtype=np.float32)[None, :] / N).astype(np.float32))
    assert np.array_equal(got[0], want), field


def test_against_torch_sort_the_float_fold_and_amin(ch, torch_mod, wide):
    """References that share nothing with the mirror: torch.sort of the int32 keys along the frame axis on the device, one
    case per field, signs mixed; rank A - 1 against [..., 0] of fold_mag_f32 at the same group; rank 0 against torch.amin on
    finite data that is not negative."""
    torch = torch_mod
    rng = np.random.default_rng(2711)
    signs = rng.choice([-1.0, 1.0], size=wide.shape).astype(np.float32)
    x = to_device(torch, wide * signs)
    for field, A, ranks in ((None, 15, [7, 0, 14, 3, 7]), ("peak", 64, [31, 63, 0, 40]), ("power", 128, [0, 127, 63, 64, 1, 126, 5, 100])):
        xs = x[:G * A]
        want = torch.sort((xs.view(torch.int32) & 0x7FFFFFFF).view(G, A, N), dim=1).values[:, ranks]
        other = torch.roll(xs, 1, 0)                              # the float that is not the point: another row's values
        t = xs if field is None else torch.stack([xs, other] if field == "peak" else [other, xs], dim=2).contiguous()
        assert torch.equal(ch.hold_ranks(t, ranks, A, field=field).view(torch.int32), want), field
    for A in (2, 16, 128):
        xs = x[:G * A]
        peak = ch.fold_mag_f32(xs, group=A)[..., 0].contiguous()
        assert torch.equal(ch.hold_ranks(xs, [A - 1], A)[:, 0].view(torch.int32), peak.view(torch.int32)), A
    pos = to_device(torch, wide)
    for A in (3, 16, 100):
        low = torch.amin(pos[:G * A].view(G, A, N), dim=1)
        assert torch.equal(ch.hold_ranks(pos[:G * A], [0], A)[:, 0].view(torch.int32), low.view(torch.int32)), A


def test_a_group_depends_on_its_own_rows_and_its_own_float(ch, torch_mod, wide):
    """A group's output is unchanged when every other group is NaN, and when the other float of the records is NaN or inf."""
    torch = torch_mod
    for A, ranks in ((5, [0, 2, 4]), (40, [0, 20, 39, 7])):
        pts = wide[:G * A]
        want = _same(_traces(ch, torch, to_device(torch, pts), ranks, A), pts, ranks, A, A)
        for g in range(G):
            loud = np.full_like(pts, np.nan)
            loud[g * A:(g + 1) * A] = pts[g * A:(g + 1) * A]
            got = _traces(ch, torch, to_device(torch, loud), ranks, A)
            assert np.array_equal(got[g], want[g]) and (np.delete(got, g, axis=0) == 0x7FC00000).all(), (A, g)
        for field, at in (("peak", 0), ("power", 1)):
            for other in (np.nan, np.inf, -np.inf):
                rec = np.full(pts.shape + (2,), other, np.float32)
                rec[..., at] = pts
                assert np.array_equal(_traces(ch, torch, to_device(torch, rec), ranks, A, field=field), want), (A, field, other)


def test_the_output_rows_are_magnitude_rows(ch, torch_mod):
    """Composition: order_stats and find_peaks on out.view(G * q, N) equal their mirrors on the mirror's rows -- the output
    really is layout 0."""
    from fpga_real_time_fft_analyzer_amd import frames
    torch = torch_mod
    A, ranks = 5, [0, 2, 4]
    ch.set_filter_mode(0xB1)
    x = _inputs(torch, _tones(2 * A, 2712))["int16"]
    mag = ch.process_f32(x, out_kind="mag_full")
    out = ch.hold_ranks(mag, ranks, A)
    rows = frames.holds_of_rows(mag.cpu().numpy(), ranks, A).reshape(2 * 3, N)
    assert np.array_equal(bits(out.cpu().numpy()).reshape(6, N), bits(rows))
    flat = out.view(2 * 3, N)
    stats = ch.order_stats(flat, [0, N - 1, N // 2])
    assert np.array_equal(bits(stats.cpu().numpy()), bits(frames.ranks_of_rows(rows, [0, N - 1, N // 2])))
    got_mag, got_bin, got_count = ch.find_peaks(flat, k=4, threshold=1.0)
    want_mag, want_bin, want_count = frames.peaks_of_rows(rows, 4, 1.0)
    assert np.array_equal(bits(got_mag.cpu().numpy()), bits(want_mag)) and np.array_equal(got_bin.cpu().numpy(), want_bin)
    assert np.array_equal(got_count.cpu().numpy(), want_count) and (want_bin[:, 0] == 1200).all()
    # the median of a stationary tone is the tone, between its min hold and its max hold
    assert (out[:, 0, 1200] <= out[:, 1, 1200]).all().item() and (out[:, 1, 1200] <= out[:, 2, 1200]).all().item()


@pytest.mark.parametrize("A", [5, 16])
def test_hold_f32(ch, torch_mod, A):
    """hold_f32 equals hold_ranks(process_f32(x, out_kind='mag_full')) bit for bit for float32, int16 and packed input at
    B = 2 A, with the cached workspace and with one given; it passes the checks of overlap, profiling and graph capture; every
    refusal comes before anything is launched."""
    from fpga_real_time_fft_analyzer_amd import frames
    from fpga_real_time_fft_analyzer_amd.abi import SpecanError
    torch = torch_mod
    ch.set_filter_mode(0xB1)
    B, qs = 2 * A, [0.0, 0.5, 1.0, 0.9]
    ranks = [frames.rank_of_quantile(v, A) for v in qs]
    assert ranks == ([0, 2, 4, 3] if A == 5 else [0, 7, 15, 13])
    forms = _inputs(torch, _tones(B, 2713 + A))
    for form, x in forms.items():
        ref = ch.hold_ranks(ch.process_f32(x, out_kind="mag_full").clone(), ranks, A).clone()
        got = ch.hold_f32(x, qs, A)                               # the cached workspace
        assert tuple(got.shape) == (2, 4, N) and torch.equal(got.view(torch.int32), ref.view(torch.int32)), form
        work = torch.full((B + 1, N), 3.0, dtype=torch.float32, device="cuda")
        out = torch.zeros((2, 4, N), dtype=torch.float32, device="cuda")
        res = ch.hold_f32(x, qs, A, work=work, out=out)
        assert res.data_ptr() == out.data_ptr() and torch.equal(out.view(torch.int32), ref.view(torch.int32)), form
        assert (work[B] == 3.0).all().item()
        med = ch.hold_f32(x, group=A)                             # the default: the lower median, one trace
        assert tuple(med.shape) == (2, 1, N) and torch.equal(med[:, 0].view(torch.int32), ref[:, 1].view(torch.int32)), form
    x = forms["int16"]
    ref = ch.hold_ranks(ch.process_f32(x, out_kind="mag_full").clone(), ranks, A).clone()
    ch.hold_f32(x, qs, A)                                         # the cached workspace, before the capture
    check_overlap_profiling_and_graph_capture(torch, ch, lambda o: ch.hold_f32(x, qs, A, out=o), ref)
    # refusals, before any launch: the workspace and the out keep what they held
    work = torch.full((B, N), 3.0, dtype=torch.float32, device="cuda")
    out = torch.full((2, 4, N), -2.0, dtype=torch.float32, device="cuda")
    for code, args, kw in ((SA_EINVAL, (x,), dict(group=1)), (SA_EINVAL, (x,), dict(q=1.5)), (SA_EINVAL, (x,), dict(q=[0.5] * 9)),
                           (SA_EINVAL, (x.double(),), {}), (SA_ESHAPE, (x[:, :100],), {}), (SA_ESHAPE, (x[:B - 1],), {}),
                           (SA_ESHAPE, (x,), dict(out=torch.zeros((2, 3, N), dtype=torch.float32, device="cuda"))),
                           (SA_ESHAPE, (x,), dict(out=torch.zeros((2, 4, N), dtype=torch.int32, device="cuda"))),
                           (SA_ESHAPE, (x,), dict(out=torch.zeros((2, 4, N), dtype=torch.float32))),
                           (SA_ESHAPE, (x,), dict(work=torch.empty((B - 1, N), dtype=torch.float32, device="cuda"))),
                           (SA_ESHAPE, (x,), dict(work=torch.empty((B, N), dtype=torch.float64, device="cuda")))):
        with pytest.raises(SpecanError) as e:
            ch.hold_f32(*args, **dict(dict(q=qs, group=A, work=work, out=out), **kw))
        torch.cuda.synchronize()
        assert e.value.code == code and (out == -2.0).all().item() and (work == 3.0).all().item(), kw


def _c_ranks(values):
    return (ctypes.c_int32 * len(values))(*values)


def test_the_c_entry_point(ch, torch_mod, wide):
    """Through ctypes: exactly the output's bytes are written; each class of refusal returns its code -- that of sa_hold_check
    for the same arguments --, sets sa_hold_last_error and leaves a sentinel-filled `out` untouched; rows = 0 is SA_OK with
    null pointers; the error text is "" after a good call."""
    from fpga_real_time_fft_analyzer_amd import abi
    from fpga_real_time_fft_analyzer_amd.abi import SpecanError
    torch = torch_mod
    L = abi.hold_lib()
    stream = torch.cuda.current_stream().cuda_stream
    A, R, guard = 3, 6, 4096
    x = to_device(torch, wide[:R])
    for ranks in ([1], [0, 2, 1, 1, 0], [2, 1, 0, 2, 1, 0, 2, 1]):
        q = len(ranks)
        n_out = (R // A) * q * N * 4
        out = torch.full((n_out + guard,), 0xFF, dtype=torch.uint8, device="cuda")
        assert L.sa_hold_f32(x.data_ptr(), 0, out.data_ptr(), R, A, q, _c_ranks(ranks), stream) == SA_OK
        assert L.sa_hold_last_error() == b""
        torch.cuda.synchronize()
        assert (out[n_out:] == 0xFF).all().item()
        got = out[:n_out].cpu().numpy().view(np.uint32).reshape(R // A, q, N)
        assert (got != 0xFFFFFFFF).all()                          # every word was written: no key of a point is all ones
        _same(got, wide[:R], ranks, A, ("C call", q))
    q, ranks = 3, [0, 1, 2]
    n_out = (R // A) * q * N * 4
    out = torch.full((n_out + guard,), 0xFF, dtype=torch.uint8, device="cuda")
    flat = torch.zeros((R * N + 64,), dtype=torch.float32, device="cuda")
    before = flat.clone()
    p_in, p_out = flat.data_ptr(), out.data_ptr()
    for tag, args, code, words in (
            ("in 4 bytes off", (p_in + 4, 0, p_out, R, A, q, ranks), SA_EINVAL, "`in` must be 16-byte aligned"),
            ("out 4 bytes off", (p_in, 0, p_out + 4, R, A, q, ranks), SA_EINVAL, "`out` must be 16-byte aligned"),
            ("out inside in", (p_in, 0, p_in + R * N * 4 - 16, R, A, q, ranks), SA_EINVAL, "overlap"),
            ("records read twice as much", (p_in, 2, p_in + R * N * 4, R, A, q, ranks), SA_EINVAL, "overlap"),
            ("NULL", (p_in, 0, 0, R, A, q, ranks), SA_EINVAL, "NULL"),
            ("q 9", (p_in, 0, p_out, R, A, 9, ranks + [0] * 6), SA_EINVAL, "q must"),
            ("field 3", (p_in, 3, p_out, R, A, q, ranks), SA_EINVAL, "field"),
            ("group 1", (p_in, 0, p_out, R, 1, q, [0, 0, 0]), SA_EINVAL, "group must be 2..128"),
            ("group 129", (p_in, 0, p_out, 129, 129, q, ranks), SA_EINVAL, "group must be 2..128"),
            ("a rank at the group", (p_in, 0, p_out, R, A, q, [0, 1, 3]), SA_EINVAL, "ranks[2] = 3"),
            ("a negative rank", (p_in, 0, p_out, R, A, q, [0, -1, 2]), SA_EINVAL, "ranks[1] = -1"),
            ("rows no multiple", (p_in, 0, p_out, R - 1, A, q, ranks), SA_ESHAPE, "the rows (5) must be a multiple of 3"),
            ("negative rows", (p_in, 0, p_out, -1, A, q, ranks), SA_ESHAPE, "negative")):
        a_in, field, a_out, rows, group, qq, rk = args
        assert L.sa_hold_check(field, a_in, a_out, rows, group, qq, _c_ranks(rk)) == code, tag
        assert L.sa_hold_f32(a_in, field, a_out, rows, group, qq, _c_ranks(rk), stream) == code, tag
        assert words in L.sa_hold_last_error().decode(), (tag, L.sa_hold_last_error())
    assert L.sa_hold_f32(p_in, 0, p_out, R, A, q, None, stream) == SA_EINVAL and b"NULL ranks" in L.sa_hold_last_error()
    torch.cuda.synchronize()
    assert (out == 0xFF).all().item() and torch.equal(flat, before)
    assert L.sa_hold_f32(0, 0, 0, 0, A, q, _c_ranks(ranks), stream) == SA_OK and L.sa_hold_last_error() == b""
    # `out` right behind `in`: touching is fine
    packed = torch.zeros((R * N * 4 + n_out,), dtype=torch.uint8, device="cuda")
    packed[:R * N * 4] = x.view(torch.uint8).view(-1)
    base = packed.data_ptr()
    assert L.sa_hold_f32(base, 0, base + R * N * 4, R, A, q, _c_ranks(ranks), stream) == SA_OK
    torch.cuda.synchronize()
    _same(packed[R * N * 4:].cpu().numpy().view(np.uint32).reshape(R // A, q, N), wide[:R], ranks, A, "touching")
    # through the wrapper: shapes and dtypes before any device call
    for code, args, kw in ((SA_ESHAPE, (x[:, :N // 2], [0], A), {}), (SA_EINVAL, (x.double(), [0], A), {}),
                           (SA_ESHAPE, (x, [0], A), dict(field="peak")), (SA_ESHAPE, (x[:5], [0], A), {}),
                           (SA_ESHAPE, (x, [0, 1], A), dict(out=torch.empty((2, 3, N), dtype=torch.float32, device="cuda"))),
                           (SA_ESHAPE, (x, [0, 1], A), dict(out=torch.empty((2, 2, N), dtype=torch.int32, device="cuda"))),
                           (SA_ESHAPE, (x, [0, 1], A), dict(out=torch.empty((2, 2, N), dtype=torch.float32))),
                           (SA_EINVAL, (x.cpu(), [0], A), {})):
        with pytest.raises(SpecanError) as e:
            ch.hold_ranks(*args, **kw)
        assert e.value.code == code, (args[0].shape, kw)
    assert ch.hold_ranks(torch.empty((0, N), dtype=torch.float32, device="cuda"), [0, 1], 2).shape == (0, 2, N)
    mine = torch.zeros((2, 3, N), dtype=torch.float32, device="cuda")
    assert ch.hold_ranks(x, ranks, A, out=mine).data_ptr() == mine.data_ptr()
    _same(bits(mine.cpu().numpy()), wide[:R], ranks, A, "out=")
    assert "libspecan_hold.so" in open("/proc/self/maps").read()


def draws(seed=2714, n=32):
    """n draws of (A, G <= 4, ranks, field): the first fifteen walk every class with every field, the rest are free; q = 1
    and q = 8 are forced once each.  Prints what the draws cover."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        amax = CLASSES[i % 5] if i < 15 else int(rng.choice(CLASSES))
        A = int(rng.integers(max(2, amax // 2 + 1) if amax > 8 else 2, amax + 1))
        field = FIELDS[(i // 5) % 3] if i < 15 else FIELDS[int(rng.integers(3))]
        q = 1 if i == 15 else 8 if i == 16 else int(rng.integers(1, 9))
        out.append((A, int(rng.integers(1, 5)), [int(v) for v in rng.integers(0, A, q)], field))
    print("draws cover classes", sorted({hold_class(a) for a, _, _, _ in out}), "fields", sorted({str(f) for _, _, _, f in out}),
          "q", sorted({len(r) for _, _, r, _ in out}), "classes x fields", len({(hold_class(a), f) for a, _, _, f in out}))
    return out


def test_drawn_sweep(ch, torch_mod, wide):
    """One seed, 32 draws of (A, G, ranks, field), each held to the mirror on rows drawn from the wide fixture."""
    cases = draws()
    assert {(hold_class(a), f) for a, _, _, f in cases} == {(c, f) for c in CLASSES for f in FIELDS}
    assert {1, 8} <= {len(r) for _, _, r, _ in cases} and len(cases) == 32
    rng = np.random.default_rng(2715)
    for A, groups, ranks, field in cases:
        pts = wide[rng.permutation(wide.shape[0])[:groups * A]]
        x = to_device(torch_mod, records_of(pts, field))
        _same(_traces(ch, torch_mod, x, ranks, A, field=field), pts, ranks, A, (A, groups, ranks, field))
