"""CPU: the signal list (include/specan_signals.h: sa_signals_f32 of libspecan_signals.so) without a GPU -- the numpy mirror
frames.signals_of_rows against a bin-by-bin restatement of the definition written here, against frames.bands_of_rows,
frames.ranks_of_rows and frames.hist_of_rows, and on the header's examples; the header against the library's exports and the
binding table; the argument check as a pure function and as a stand-alone program under the host sanitizers.  What it
links and its resource remarks: tests/test_reduction_libraries_cpu.py; the refusals of the two wrappers:
tests/test_reductions_wrappers_cpu.py.

The rows made here are the data of tests/test_gpu_f32_signals.py too, which holds the device against the mirror bit for bit."""
import ctypes
import functools
import inspect
import itertools
import os
import re

import numpy as np
import pytest

from conftest import N
from kernel_inventory import inventory
from native import INCLUDE, compiles_as_c, declared, exported, standalone_checks
from reduction_libraries import BASE, FIELDS, SA_EINVAL, SA_ESHAPE, SA_OK, _shared, bits, built, records_of
from test_f32_bands_cpu import noise_rows, same_bits

HEADER = os.path.join(INCLUDE, "specan_signals.h")
NAMES = ["sa_signals_check", "sa_signals_f32", "sa_signals_last_error", "sa_signals_version"]
KERNELS = {f"signals_f32_kernel<{f}>" for f in range(3)}
WORDS = ("start", "stop", "peak", "peak_bin")
# the ownership boundaries of csrc/signals_f32.hip: a 16-byte unit of records (2 bins) that is no lane's (14), a lane's four
# bins and a unit of magnitudes (8), a word of the on-mask (64), a wave's tile (256), a round (1024), and later ones of each
BOUNDS = (8, 14, 64, 256, 1024, 1280, 4096, 8192, 12288, 16128)
GAPS = (1, 3, 63, 64, 65, 300)


def signals(pts, field=None, **kw):
    from fpga_real_time_fft_analyzer_amd import frames
    return frames.signals_of_rows(records_of(pts, field), field=field, **kw)


def same_records(a, b):
    """None where two SIGNAL arrays are equal bit for bit (a NaN power by position, the floats as words), else what differs"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return f"{a.dtype} {a.shape} against {b.dtype} {b.shape}"
    if not same_bits(a["power"], b["power"]):
        return "power"
    for name in WORDS:
        x, y = np.ascontiguousarray(a[name]).view(np.int32), np.ascontiguousarray(b[name]).view(np.int32)
        if not np.array_equal(x, y):
            return f"{name}: rows {np.argwhere((x != y).reshape(len(a), -1).any(axis=1)).ravel()[:5].tolist()}"
    return None


def same_result(got, want):
    """None where (records, stats) pairs are equal bit for bit, else what differs"""
    bad = same_records(got[0], want[0])
    if bad is None and not np.array_equal(got[1], want[1]):
        rows = np.argwhere((got[1] != want[1]).any(axis=1)).ravel()[:5].tolist()
        bad = f"stats: rows {rows}: {got[1][rows].tolist()} against {want[1][rows].tolist()}"
    return bad


def brute(pts, k, threshold, lo, hi, gap, min_width, field=None):
    """The definition of the header, bin by bin in Python loops: (start, stop, peak bits, peak_bin) of the first k kept
    segments of every row, and the row's (count, occupied, covered).  ``threshold`` is a float or an array [R]."""
    keys = (np.ascontiguousarray(pts).view(np.uint32) & 0x7FFFFFFF).tolist()
    thr = np.broadcast_to(np.asarray(threshold, np.float32), (len(pts),)).copy()
    out = []
    for r, u in enumerate(keys):
        T = int(thr[r:r + 1].view(np.uint32)[0]) & 0x7FFFFFFF
        on = [lo <= i < hi and u[i] > 0 and u[i] >= T for i in range(N)]
        closed = list(on)
        last = None                                                # the on bin before the off run that is being walked
        i = 0
        while i < N:
            if on[i]:
                last = i
                i += 1
                continue
            j = i
            while j < N and not on[j]:
                j += 1
            if last is not None and j < N and j - last - 1 <= gap:  # an on bin at either end, and short enough
                for b in range(i, j):
                    closed[b] = True
            i = j
        segs, i = [], 0
        while i < N:
            if closed[i]:
                j = i
                while j < N and closed[j]:
                    j += 1
                segs.append((i, j))
                i = j
            else:
                i += 1
        kept = [(a, b) for a, b in segs if b - a >= min_width]
        recs = []
        for a, b in kept[:k]:
            top = max(u[a:b])
            recs.append((a, b, top, a + u[a:b].index(top)))
        out.append((recs, (len(kept), sum(on), sum(b - a for a, b in kept))))
    return out


def against_brute(pts, field=None, **kw):
    """the mirror on ``pts`` against brute(): every word, and the power against frames.bands_of_rows of [start, stop)"""
    from fpga_real_time_fft_analyzer_amd import frames
    args = dict(k=16, threshold=0.0, lo=0, hi=N, gap=0, min_width=1)
    args.update(kw)
    rec, stats = signals(pts, field, **args)
    want = brute(pts, **args)
    for r, (recs, st) in enumerate(want):
        assert stats[r].tolist() == list(st), (r, kw, stats[r], st)
        m = len(recs)
        assert (rec["start"][r, m:] == -1).all() and (rec["stop"][r, m:] == -1).all() and (rec["peak_bin"][r, m:] == -1).all()
        assert not rec["peak"][r, m:].view(np.uint32).any() and not rec["power"][r, m:].view(np.uint64).any()
        for j, (a, b, top, at) in enumerate(recs):
            got = rec[r, j]
            assert (got["start"], got["stop"], int(rec["peak"][r, j:j + 1].view(np.uint32)[0]), got["peak_bin"]) == (a, b, top, at), (r, j, kw)
            power, _ = frames.bands_of_rows(records_of(pts[r:r + 1], field), [(a, b)], field=field)
            assert same_bits(power[0, :1], rec["power"][r, j:j + 1]), (r, j, kw)
    return rec, stats


# ------------------------------------------------------------------------------------------------------------- the rows
@functools.lru_cache(maxsize=None)
def edge_rows():
    """8 rows over a floor below 0.1, the signals 1..2: segments that end at, start at, straddle, lie one bin below and one
    bin at every boundary of BOUNDS; bins 0 and 16383 with a segment over two rounds; on bins at 99, 100, 15999 and 16000 (for
    the range [100, 16000)); one segment from 250 to 1030"""
    rng = np.random.default_rng(2501)
    pts = (0.1 * rng.random((8, N))).astype(np.float32)
    sig = (1.0 + rng.random((8, N))).astype(np.float32)
    spans = [[(b - 3, b) for b in BOUNDS], [(b, b + 3) for b in BOUNDS], [(b - 2, b + 2) for b in BOUNDS], [(b - 1, b) for b in BOUNDS],
             [(b, b + 1) for b in BOUNDS], [(0, 1), (1000, 3000), (N - 1, N)], [(99, 101), (15999, 16001), (5000, 5001)],
             [(250, 1030), (N - 2, N)]]
    for r, row in enumerate(spans):
        for a, b in row:
            pts[r, a:b] = sig[r, a:b]
    return _shared(pts)


@functools.lru_cache(maxsize=None)
def gap_rows():
    """6 rows of zeros, one per gap g of GAPS, holding pairs of on bins with exactly g off bins between them across a tile
    border (768) and a word border that is no tile border (6464), with g + 1 across 2048 and at 9000; an on bin at 12000, just
    outside the range [12001, 14001), with the first on bin inside g bins further, and the last on bin inside g bins before an
    on bin at 14001: a gap that reaches to lo and one that reaches to hi"""
    pts = np.zeros((len(GAPS), N), np.float32)
    for r, g in enumerate(GAPS):
        for p, width in ((767 - g // 2, g), (6463 - g // 2, g), (2047 - (g + 1) // 2, g + 1), (9000, g + 1)):
            pts[r, p] = 1.0 + r
            pts[r, p + width + 1] = 2.0 + r
        pts[r, [12000, 12001 + g, 14000 - g, 14001]] = 3.0
    return _shared(pts)


@functools.lru_cache(maxsize=None)
def many_rows():
    """7 rows: 0 alternating on / off from bin 0 (8192 segments); 1 segments of the widths 1, 2, 3, 1, ... one off bin apart;
    2 every bin on; 3 all zero; 4 all NaN; 5 |N(0,1)| noise; 6 alternating from bin 1"""
    rng = np.random.default_rng(2502)
    pts = np.zeros((7, N), np.float32)
    amp = (1.0 + rng.random(N)).astype(np.float32)
    pts[0, 0::2] = amp[0::2]
    i, w = 0, 0
    while i < N:
        width = 1 + w % 3
        pts[1, i:i + width] = amp[i:i + width]
        i, w = i + width + 1, w + 1
    pts[2] = amp
    pts[4] = np.nan
    pts[5] = noise_rows()[5]
    pts[6, 1::2] = amp[1::2]
    return _shared(pts)


@functools.lru_cache(maxsize=None)
def special_rows():
    """6 rows: 0 negative points and -0.0; 1 denormals alone, some larger; 2 +inf points in a finite floor; 3 a NaN inside a
    segment and one alone; 4 |N(0,1)| noise; 5 equal peaks in one segment"""
    rng = np.random.default_rng(2503)
    pts = (0.1 * rng.random((6, N))).astype(np.float32)
    pts[0, 500:520] = -3.0
    pts[0, 1::2] *= -1.0
    pts[0, 2000:2600] = -0.0
    pts[0, 2300] = -2.0
    pts[1] = (1e-45 * rng.integers(1, 9, N)).astype(np.float32)
    pts[1, 4321:4330] = 1e-38
    pts[2, [1000, 1001, 6000]] = np.inf
    pts[3, 700:710] = 2.0
    pts[3, 705] = np.nan
    pts[3, 9000] = np.nan
    pts[4] = noise_rows()[4]
    pts[5, 3000:3010] = 4.0
    pts[5, [3003, 3007]] = 9.0
    return _shared(pts)


# ------------------------------------------------------------------------------------------------------------- the mirror
def test_examples_of_the_header():
    pts = np.zeros((1, N), np.float32)
    pts[0, [10, 11, 14]] = 1.0
    for kw, recs, stats in ((dict(), [(10, 12, 1.0, 10, 2.0), (14, 15, 1.0, 14, 1.0)], (2, 3, 3)),
                            (dict(gap=2), [(10, 15, 1.0, 10, 3.0)], (1, 3, 5)),
                            (dict(min_width=2), [(10, 12, 1.0, 10, 2.0)], (1, 3, 2))):
        for field in FIELDS:
            rec, st = signals(pts, field, k=3, threshold=0.5, **kw)
            assert rec[0].tolist() == recs + [(-1, -1, 0.0, -1, 0.0)] * (3 - len(recs)) and tuple(st[0]) == stats, (kw, field)


def test_constructed_rows_against_the_definition():
    """Every boundary of the kernel's ownership, bin by bin: the full range, a range that cuts segments, k below and above the
    number of segments, min_width 2, 3 and 4."""
    pts = edge_rows()
    for field in FIELDS:
        rec, stats = against_brute(pts, field, k=32, threshold=0.5)
        assert stats[:5, 0].tolist() == [len(BOUNDS)] * 5 and stats[5:, 0].tolist() == [3, 3, 2]
        assert rec["start"][0, :len(BOUNDS)].tolist() == [b - 3 for b in BOUNDS] and rec["stop"][4, :len(BOUNDS)].tolist() == [b + 1 for b in BOUNDS]
    _, stats = against_brute(pts, k=4, threshold=0.5, lo=100, hi=16000)
    assert stats[6].tolist() == [3, 3, 3] and stats[5].tolist() == [1, 2000, 2000]     # the on bins at 99 and 16000 do not exist
    against_brute(pts, k=32, threshold=0.5, lo=1025, hi=8191)
    for min_width in (2, 3, 4):
        _, stats = against_brute(pts, k=7, threshold=0.5, min_width=min_width)
        assert stats[3, 0] == stats[4, 0] == 0 and stats[2, 0] == len(BOUNDS)
    against_brute(pts, k=32, threshold=0.0)                       # every non-zero bin: one segment
    against_brute(pts, k=32, threshold=float("inf"))


def test_gaps_against_the_definition():
    """Gaps of exactly g and g + 1 bins across word and tile borders: the first are bridged, the others are not; bridged bins
    hold zeros and are in the band; a gap that reaches to lo or to hi is not bridged."""
    pts = gap_rows()
    for r, g in enumerate(GAPS):
        rec, stats = against_brute(pts[r:r + 1], k=32, threshold=0.5, gap=g)
        assert stats[0].tolist() == [8, 12, 4 * (g + 2) + 4], (g, stats)            # the gaps of g bins are bridged, those of g + 1 not
        assert (768 > rec["start"][0, 0] == 767 - g // 2) and rec["stop"][0, 0] == 767 - g // 2 + g + 2 > 768
        assert rec["power"][0, 0] == (1.0 + r) ** 2 + (2.0 + r) ** 2
        rec, stats = against_brute(pts[r:r + 1], k=32, threshold=0.5, gap=g, lo=12001, hi=14001)
        assert stats[0].tolist() == [2, 2, 2], (g, stats)
        rec, stats = against_brute(pts[r:r + 1], k=32, threshold=0.5, gap=g, lo=12000, hi=14002)
        assert stats[0].tolist() == [2, 4, 2 * (g + 2)], (g, stats)
    for field in FIELDS:
        against_brute(pts, field, k=32, threshold=0.5, gap=64, min_width=3)
        against_brute(pts, field, k=32, threshold=0.5, gap=N - 1)


def test_many_segments_against_the_definition():
    pts = many_rows()
    for k in (1, 32):
        rec, stats = against_brute(pts, k=k, threshold=0.5)
        assert stats[0].tolist() == [8192, 8192, 8192] and stats[6].tolist() == [8192, 8192, 8192] and stats[2].tolist() == [1, N, N]
        assert stats[3].tolist() == [0, 0, 0] and stats[4].tolist() == [1, N, N] and np.isnan(rec["power"][4, 0])
        assert rec["start"][0, :k].tolist() == [2 * j for j in range(k)] and (stats[[0, 1, 5, 6], 0] > k).all()
    for min_width in (2, 3):
        rec, stats = against_brute(pts, k=32, threshold=0.5, min_width=min_width)
        assert stats[0, 0] == 0 and 32 < stats[1, 0] < 8192 // 2 and np.diff(rec["start"][1]).max() >= 6      # a dropped one between kept ones
    rec, stats = against_brute(pts, k=32, threshold=0.5, gap=1)
    assert stats[0].tolist() == [1, 8192, N - 1] and stats[6].tolist() == [1, 8192, N - 1] and stats[1, 0] == 1


def test_random_rows_against_the_definition():
    """Random on-densities, ranges, gaps, widths and k, all three fields, a threshold per row."""
    rng = np.random.default_rng(2504)
    for trial in range(12):
        p = rng.choice([0.002, 0.05, 0.5, 0.95])
        pts = np.where(rng.random((2, N)) < p, 1.0 + rng.random((2, N)), 0.3 * rng.random((2, N))).astype(np.float32)
        lo, hi = int(rng.integers(0, 600)), int(rng.integers(15000, N + 1))
        thr = np.array([0.5, 1.5], np.float32) if trial % 2 else 0.5
        against_brute(pts, FIELDS[trial % 3], k=int(rng.choice([1, 5, 32])), threshold=thr, lo=lo, hi=hi,
                      gap=int(rng.choice([0, 1, 2, 7, 64, 1000])), min_width=int(rng.choice([1, 2, 5, 100])))


def test_specials_and_thresholds_per_row():
    """-0.0 is never on, a negative point counts by its magnitude, denormals are kept, +inf is a point like another; a
    threshold of 0 passes every non-zero bin, +inf only infinities and NaNs, a NaN only NaNs, a negative one its magnitude."""
    pts = special_rows()
    for field in FIELDS:
        rec, stats = against_brute(pts, field, k=32, threshold=0.5)
        assert (rec["start"][0, 0], rec["stop"][0, 0], rec["peak"][0, 0], rec["peak_bin"][0, 0]) == (500, 520, 3.0, 500)
        assert rec["start"][0, 1] == 2300 and stats[1].tolist() == [0, 0, 0] and np.isinf(rec["power"][2, 0]) and rec["stop"][2, 0] == 1002
        assert rec["peak_bin"][3, 0] == 705 and np.isnan(rec["peak"][3, 0]) and np.isnan(rec["power"][3, 0]) and rec["peak_bin"][5, 0] == 3003
    rec, stats = against_brute(pts, k=32, threshold=0.0)
    assert stats[0].tolist() == [3, N - 599, N - 599] and stats[1].tolist() == [1, N, N]
    assert 0 < rec["power"][1, 0] < 1e-70 and rec["peak_bin"][1, 0] == 4321
    against_brute(pts, k=32, threshold=1e-44)
    thr = np.array([0.0, np.inf, np.nan, -1.5, 0.0, -np.inf], np.float32)
    for rows, t in ((slice(0, 6), thr), (slice(2, 4), thr[1:3]), (slice(2, 4), thr[2:0:-1].copy())):
        rec, stats = against_brute(pts[rows], k=32, threshold=t, gap=1)
    rec, stats = against_brute(pts[[2, 3, 3, 4]], k=32, threshold=np.array([np.inf, np.inf, np.nan, -2.5], np.float32))
    assert stats[0].tolist() == [2, 3, 3] and stats[1].tolist() == [2, 2, 2] == stats[2].tolist() and stats[3, 0] > 10
    assert rec["start"][2, :2].tolist() == [705, 9000]


def test_agreements_with_the_other_mirrors():
    """power is bands_of_rows of [start, stop), peak the top rank of ranks_of_rows over it; with gap 0, min_width 1 and a
    non-zero threshold occupied == covered == the upper-level counts of hist_of_rows with that one edge."""
    from fpga_real_time_fft_analyzer_amd import frames
    pts = noise_rows()[:6]
    for field, threshold in itertools.product(FIELDS, (2.5, 3.5)):
        x = records_of(pts, field)
        rec, stats = frames.signals_of_rows(x, k=16, threshold=threshold, field=field)
        assert (stats[:, 0] >= 1).all() and (stats[:, 1] == stats[:, 2]).all()
        hist = frames.hist_of_rows(pts, [threshold], group=1, bucket=1)              # [R, N, 2]
        assert stats[:, 1].tolist() == hist[:, :, 1].sum(axis=1).tolist()
        for r in range(len(pts)):
            for j in range(min(int(stats[r, 0]), 16)):
                a, b = int(rec["start"][r, j]), int(rec["stop"][r, j])
                power, _ = frames.bands_of_rows(x[r:r + 1], [(a, b)], field=field)
                top = frames.ranks_of_rows(x[r:r + 1], [b - a - 1], a, b, field=field)
                assert same_bits(power[0], rec["power"][r, j:j + 1]) and top[0, 0] == rec["peak"][r, j]
    wide, stats = frames.signals_of_rows(pts, k=4, threshold=2.5, gap=40, min_width=3)
    assert (stats[:, 0] >= 1).all() and (stats[:, 2] > stats[:, 1]).all()
    for r in range(len(pts)):
        a, b = int(wide["start"][r, 0]), int(wide["stop"][r, 0])
        assert same_bits(frames.bands_of_rows(pts[r:r + 1], [(a, b)])[0][0], wide["power"][r, :1])


def test_arguments_of_the_mirror():
    from fpga_real_time_fft_analyzer_amd import frames
    pts = np.zeros((1, N), np.float32)
    assert frames._signals_args(16, 0, N, 0, 1, None) == (16, 0, N, 0, 1)
    assert frames._signals_args(np.int64(32), 5, 6, N - 1, N, "power") == (32, 5, 6, N - 1, N)
    bad = [dict(k=0), dict(k=33), dict(k=2.0), dict(k=True), dict(k=None), dict(lo=-1), dict(lo=5, hi=5), dict(lo=6, hi=5),
           dict(hi=N + 1), dict(lo=0.0), dict(hi="5"), dict(gap=-1), dict(gap=N), dict(gap=1.0), dict(gap=False), dict(min_width=0),
           dict(min_width=N + 1), dict(min_width=2.0), dict(threshold=-1.0), dict(threshold=-0.0), dict(threshold=float("nan")),
           dict(threshold="1"), dict(threshold=True), dict(threshold=None), dict(threshold=[0.5]),
           dict(threshold=np.zeros(2, np.float32)), dict(threshold=np.zeros(1, np.float64)), dict(threshold=np.zeros((1, 1), np.float32)),
           dict(field="mag"), dict(field=0), dict(field=["peak"])]
    for kw in bad:
        with pytest.raises(ValueError):
            frames.signals_of_rows(pts, **kw)
    for wrong in (pts.astype(np.float64), pts[0], np.zeros((1, N, 2), np.float32), np.zeros((1, N - 1), np.float32)):
        with pytest.raises(ValueError):
            frames.signals_of_rows(wrong)
    with pytest.raises(ValueError):
        frames.signals_of_rows(pts, field="peak")
    rec, stats = frames.signals_of_rows(np.zeros((0, N), np.float32), k=5)
    assert rec.shape == (0, 5) and stats.shape == (0, 3) and rec.dtype == frames.SIGNAL and stats.dtype == np.int32
    rec, stats = frames.signals_of_rows(np.ones((1, N, 2), np.float32), field="power", threshold=np.float32(1.0), k=1)
    assert rec[0, 0].tolist() == (0, N, 1.0, 0, float(N)) and stats[0].tolist() == [1, N, N]


# ------------------------------------------------------------------------------------------------------------ the surface
@pytest.fixture(scope="module")
def signals_lib():
    return built("signals")


GOOD = dict(rows=3, k=8, lo=0, hi=N, gap=0, min_width=1)
FAR = {"in": BASE, "thr": 0, "out": BASE + (1 << 40), "stats": BASE + (1 << 41)}


@pytest.fixture(scope="module")
def check(signals_lib):
    def call(field=0, bits=0, **kw):
        addr = {name: kw.pop(name, FAR[name]) for name in FAR}
        a = dict(GOOD, **kw)
        return signals_lib.sa_signals_check(field, addr["in"], addr["thr"], bits, addr["out"], addr["stats"], a["rows"], a["k"],
                                            a["lo"], a["hi"], a["gap"], a["min_width"])
    return call


def test_header_library_and_binding_table(signals_lib):
    """Name for name: declared in specan_signals.h = exported by libspecan_signals.so = bound in abi.SIGNALS_SIGNATURES;
    nothing is in the other tables or headers, which are what they were.  The record three times: the header's struct, the
    binding's Structure, the mirror's dtype."""
    from fpga_real_time_fft_analyzer_amd import abi, frames
    assert declared(HEADER) == NAMES
    assert [n for n in exported(abi.SIGNALS_LIB_PATH) if "sa_" in n] == NAMES
    assert sorted(abi.SIGNALS_SIGNATURES) == NAMES
    others = (abi.SIGNATURES, abi.EXT_SIGNATURES, abi.FOLD_SIGNATURES, abi.PEAKS_SIGNATURES, abi.RANK_SIGNATURES, abi.HIST_SIGNATURES,
              abi.BANDS_SIGNATURES, abi.MASK_SIGNATURES, abi.HARM_SIGNATURES)
    assert not set(NAMES) & set().union(*others)
    assert [len(t) for t in others] == [45, 5, 4, 4, 4, 4, 4, 4, 4]
    for other in ("specan.h", "specan_ext.h", "specan_fold.h", "specan_peaks.h", "specan_rank.h", "specan_hist.h", "specan_bands.h",
                  "specan_mask.h", "specan_harm.h"):
        assert not set(NAMES) & set(declared(os.path.join(INCLUDE, other))), other
    for name in NAMES:
        fn, (restype, argtypes) = getattr(signals_lib, name), abi.SIGNALS_SIGNATURES[name]
        assert fn.argtypes is not None and list(fn.argtypes) == list(argtypes), name
        assert fn.restype is restype is (ctypes.c_char_p if name == "sa_signals_last_error" else ctypes.c_int), name
    assert signals_lib.sa_signals_version() == abi.SA_SIGNALS_VERSION == 1
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", text)
    for line in ("#define SA_SIGNALS_VERSION 1", "#define SA_SIGNALS_K_MAX 32", "#define SA_SIGNALS_IN_MAG 0",
                 "#define SA_SIGNALS_IN_POINT_PEAK 1", "#define SA_SIGNALS_IN_POINT_POWER 2",
                 "int sa_signals_f32(const void *in, int field, const float *thr, float threshold, sa_signal *out, int32_t *stats, "
                 "int rows, int k, int lo, int hi, int gap, int min_width, void *stream);",
                 "int sa_signals_check(int field, uint64_t in_addr, uint64_t thr_addr, uint32_t threshold_bits, uint64_t out_addr, "
                 "uint64_t stats_addr, int rows, int k, int lo, int hi, int gap, int min_width);"):
        assert line in flat, line
    assert '#include "specan.h"' in text and "#include \"specan_bands.h\"" not in text and "#include \"specan_peaks.h\"" not in text
    assert (abi.SA_SIGNALS_IN_MAG, abi.SA_SIGNALS_IN_POINT_PEAK, abi.SA_SIGNALS_IN_POINT_POWER) == (0, 1, 2) == \
        (abi.SA_PEAKS_IN_MAG, abi.SA_PEAKS_IN_POINT_PEAK, abi.SA_PEAKS_IN_POINT_POWER)
    assert abi.SA_SIGNALS_K_MAX == 32 == frames.SIGNALS_K_MAX and frames.SIGNALS_GAP_MAX == N - 1
    assert ctypes.sizeof(abi.Signal) == 24 == frames.SIGNAL.itemsize
    assert [n for n, _ in abi.Signal._fields_] == list(frames.SIGNAL.names)
    offsets = [getattr(abi.Signal, n).offset for n, _ in abi.Signal._fields_]
    assert offsets == [frames.SIGNAL.fields[n][1] for n in frames.SIGNAL.names] == [0, 4, 8, 12, 16]
    struct = re.search(r"typedef struct \{([^}]*)\} sa_signal;", re.sub(r"/\*.*?\*/", "", text, flags=re.S)).group(1)
    assert re.findall(r"\b([a-z_]+)[,;]", struct) == list(frames.SIGNAL.names)
    assert re.findall(r"(double|int32_t|float)\s", struct) == ["int32_t", "float", "int32_t", "double"]
    assert signals_lib.sa_signals_last_error() == b""
    assert os.path.basename(abi.SIGNALS_LIB_PATH) == "libspecan_signals.so"
    assert os.path.dirname(abi.SIGNALS_LIB_PATH) == os.path.dirname(abi.LIB_PATH)
    assert list(abi.LIBRARIES)[-1] == "signals" and abi.LIBRARIES["signals"] == ("libspecan_signals.so", abi.SIGNALS_SIGNATURES)
    assert abi.signals_lib.__name__ == "signals_lib" and "specan_signals.h" in abi.signals_lib.__doc__


def test_header_compiles_as_c99_pedantic(tmp_path):
    compiles_as_c(tmp_path, '#include "specan_signals.h"\n'
                  "int use(const void *p, const float *t, sa_signal *o, int32_t *s) {"
                  " return sa_signals_f32(p, SA_SIGNALS_IN_POINT_POWER, t, 0.5f, o, s, 8, SA_SIGNALS_K_MAX, 0, SA_N, 3, 1, 0)"
                  " + sa_signals_check(SA_SIGNALS_IN_MAG, 16, 0, 0, 1 << 20, 1 << 21, 1, 1, 0, 1, 0, 1)"
                  " + sa_signals_version() - SA_SIGNALS_VERSION + (sa_signals_last_error()[0] != 0) + SA_SIGNALS_IN_POINT_PEAK - 1"
                  " + o[0].start + o[0].stop + (o[0].peak > 0) + o[0].peak_bin + (o[0].power > 0) + (int)sizeof(sa_signal); }\n")


def test_kernel_inventory(signals_lib):
    """libspecan_signals.so holds the three instantiations, one per input layout, and nothing else."""
    from fpga_real_time_fft_analyzer_amd import abi
    assert inventory(abi.SIGNALS_LIB_PATH) == KERNELS


# -------------------------------------------------------------------------------------------------------------- the check
def sizes(field, rows, k):
    return {"in": rows * 65536 * (2 if field else 1), "thr": rows * 4, "out": rows * k * 24, "stats": rows * 12}


def test_known_answers_of_the_header(check):
    n = sizes(0, 3, 8)
    assert (n["in"], n["thr"], n["out"], n["stats"]) == (196608, 12, 576, 36)
    n = sizes(2, 1, 32)
    assert (n["in"], n["out"], n["stats"]) == (131072, 768, 12)
    # in | thr | out | stats in a row, touching
    at = dict(thr=BASE + 196608, out=BASE + 196608 + 16, stats=BASE + 196608 + 16 + 576)
    assert check(0, **{"in": BASE}, **at) == SA_OK
    assert check(0, **{"in": BASE}, **dict(at, out=at["out"] - 8)) == SA_EINVAL      # the records on thr
    assert check(0, **{"in": BASE}, **dict(at, stats=at["stats"] - 4)) == SA_EINVAL  # the counts on the records
    assert check(1, **{"in": BASE}, **at) == SA_EINVAL                               # records read twice as much
    assert check(0, **{"in": BASE}, **dict(at, thr=BASE + 64)) == SA_OK              # thr inside in: both only read
    assert check(0, **{"in": BASE}, **dict(at, thr=at["out"] + 572)) == SA_EINVAL and check(0, **dict(at, thr=at["stats"] + 32)) == SA_EINVAL
    assert check(2, rows=1, k=32, **{"in": BASE, "out": BASE + 131072, "stats": BASE + 131072 + 768}) == SA_OK
    assert check(2, rows=1, k=32, **{"in": BASE, "out": BASE + 131072, "stats": BASE + 131072 + 764}) == SA_EINVAL
    assert check(2, rows=1, k=32, **{"in": BASE, "out": BASE - 768, "stats": BASE - 780}) == SA_OK
    assert check(2, rows=1, k=32, **{"in": BASE, "out": BASE - 760, "stats": BASE - 780}) == SA_EINVAL


def test_touching_and_overlapping_ranges(check):
    """Each written range right behind and right in front of every other range is fine; moved into it it is refused; `in` and
    `thr` may lie anywhere on each other; at addresses past 2^32 and near 2^47."""
    for X in (BASE + (1 << 30), (1 << 32) - 65536, 1 << 33):
        for field, rows, k in itertools.product((0, 2), (1, 5, 4096), (1, 32)):
            n = sizes(field, rows, k)
            far = {"in": X + (1 << 42), "thr": X + (1 << 43), "out": X + (1 << 44), "stats": X + (1 << 45)}
            assert check(field, rows=rows, k=k, **far) == SA_OK
            for a, b in (("out", "in"), ("stats", "in"), ("out", "stats"), ("out", "thr"), ("stats", "thr")):
                def at(pa, pb):
                    return check(field, rows=rows, k=k, **dict(far, **{a: pa, b: pb}))
                Y = X + (1 << 36)                                   # 16-byte aligned, like X
                behind = SA_OK if (Y + n[b]) % (8 if a == "out" else 4) == 0 else SA_EINVAL      # 12 bytes behind: no place for records
                assert at(Y + n[b], Y) == behind and at(Y - n[a], Y) == SA_OK, (a, b, field, rows, k)
                assert at(Y + n[b] - 8, Y) == SA_EINVAL, (a, b, field, rows, k)
                assert at(Y - n[a] + 8, Y) == SA_EINVAL, (a, b, field, rows, k)
                assert at(Y, Y) == SA_EINVAL
            for off in (0, 4, n["in"] - 4, n["in"]):
                assert check(field, rows=rows, k=k, **dict(far, thr=far["in"] + off)) == SA_OK
            for off in (1, 2, 4, 8, 12, 16, 32):
                assert check(field, rows=rows, k=k, **dict(far, **{"in": far["in"] + off})) == (SA_OK if off % 16 == 0 else SA_EINVAL)
                assert check(field, rows=rows, k=k, **dict(far, out=far["out"] + off)) == (SA_OK if off % 8 == 0 else SA_EINVAL)
                assert check(field, rows=rows, k=k, **dict(far, stats=far["stats"] + off)) == (SA_OK if off % 4 == 0 else SA_EINVAL)
                assert check(field, rows=rows, k=k, **dict(far, thr=far["thr"] + off)) == (SA_OK if off % 4 == 0 else SA_EINVAL)
            for name in ("in", "out", "stats"):
                assert check(field, rows=rows, k=k, **dict(far, **{name: 0})) == SA_EINVAL
            assert check(field, rows=rows, k=k, **dict(far, thr=0)) == SA_OK


def test_refusals_in_their_order(check, signals_lib):
    """1 negative rows, 2 the field and the parameters (also at rows 0), 3 the empty call, 4 the pointers: each refusal is
    shown to win over every later one by making the later ones wrong too."""
    NAN, NEG, NZERO, INF = 0x7FC00000, 0xBF800000, 0x80000000, 0x7F800000
    bad = [dict(field=-1), dict(field=3), dict(k=0), dict(k=33), dict(k=-2 ** 31), dict(bits=NAN), dict(bits=NEG), dict(bits=NZERO),
           dict(bits=INF + 1), dict(bits=0xFFFFFFFF), dict(lo=-1), dict(lo=5, hi=5), dict(lo=6, hi=5), dict(hi=N + 1),
           dict(lo=-2 ** 31, hi=2 ** 31 - 1), dict(gap=-1), dict(gap=N), dict(gap=2 ** 31 - 1), dict(min_width=0), dict(min_width=N + 1),
           dict(min_width=-2 ** 31)]
    wrong_ptrs = [dict(), {"in": 0, "out": 0, "stats": 0}, {"in": BASE + 1, "out": BASE + 3, "stats": BASE + 2},
                  {"in": BASE, "out": BASE, "stats": BASE}]
    for kw in [dict()] + bad:
        for p in wrong_ptrs:
            assert check(**dict(p, rows=-1, **kw)) == SA_ESHAPE, (kw, p)
            assert check(**dict(p, rows=-(1 << 31), **kw)) == SA_ESHAPE, (kw, p)
    for rows in (0, 1, 5, (1 << 31) - 1):
        for kw in bad:
            for p in wrong_ptrs:
                assert check(**dict(p, rows=rows, **kw)) == SA_EINVAL, (rows, kw, p)
    for p in wrong_ptrs:
        for field in (0, 1, 2):
            assert check(field=field, **dict(p, rows=0)) == SA_OK, p
    for p in wrong_ptrs[1:]:
        assert check(**dict(p, rows=1)) == SA_EINVAL, p
    assert check(rows=1) == SA_OK
    # with `thr` the threshold's bits are not looked at; a misaligned thr is a pointer's refusal, after the empty call
    for bits in (NAN, NEG, NZERO, 0xFFFFFFFF):
        assert check(bits=bits, thr=BASE + (1 << 42)) == SA_OK and check(bits=bits, thr=BASE + (1 << 42), rows=0) == SA_OK
    assert check(thr=BASE + (1 << 42) + 2) == SA_EINVAL and check(thr=BASE + (1 << 42) + 2, rows=0) == SA_OK
    for kw in (dict(k=1, lo=0, hi=1, gap=0, min_width=1), dict(k=32, lo=N - 1, hi=N, gap=N - 1, min_width=N), dict(field=2),
               dict(bits=INF), dict(bits=1), dict(rows=(1 << 31) - 1, k=32, **{"in": 1 << 20, "out": 1 << 62, "stats": 1 << 61})):
        assert check(**kw) == SA_OK, kw
    assert signals_lib.sa_signals_last_error() == b""             # the check alone leaves the thread's text alone


def test_standalone_program_under_host_sanitizers(tmp_path):
    """tests/cpp/test_sa_signals_check.cpp + csrc/sa_signals_check.cpp, host only, under the address and undefined-behaviour
    sanitizers when they link here (a plain build otherwise: the program's own checks still run): every refusal in its order
    with the later ones wrong too, the known answers in bytes, touching and overlapping buffers at rows up to 2^31 - 1 and
    addresses past 2^32, near 2^47 and near 2^64.  Nothing is loaded into this process."""
    assert standalone_checks(tmp_path, "test_sa_signals_check", ["sa_signals_check.cpp"]) > 30000


# ----------------------------------------------------------------------------------------------------------- the wrappers
def test_the_wrappers_surface():
    from fpga_real_time_fft_analyzer_amd import abi, chain, frames, reductions
    cls = chain.SpectrumChain
    assert list(inspect.signature(frames.signals_of_rows).parameters) == ["points", "k", "threshold", "lo", "hi", "gap", "min_width", "field"]
    assert list(inspect.signature(cls.find_signals).parameters) == ["self", "t", "k", "threshold", "lo", "hi", "gap", "min_width", "field",
                                                                    "out", "stats"]
    assert list(inspect.signature(cls.signals_f32).parameters) == ["self", "x", "k", "threshold", "factor", "q", "lo", "hi", "gap",
                                                                   "min_width", "group", "scale", "work", "out", "stats"]
    for fn in (frames.signals_of_rows, cls.find_signals, cls.signals_f32):
        sig = inspect.signature(fn).parameters
        assert (sig["k"].default, sig["lo"].default, sig["hi"].default, sig["gap"].default, sig["min_width"].default) == (16, 0, N, 0, 1)
    assert inspect.signature(cls.find_signals).parameters["threshold"].default == 0.0
    sig = inspect.signature(cls.signals_f32).parameters
    assert (sig["threshold"].default, sig["factor"].default, sig["q"].default, sig["scale"].default) == (None, None, 0.5, 1.0 / 2048.0)
    assert reductions.SIGNAL_WORDS == 6 and cls._signals_args(np.int64(32), 1.0, 0, N, 5, 2, "power") == 2
    assert callable(cls._signals_out) and cls.find_signals is reductions.Reductions.find_signals
