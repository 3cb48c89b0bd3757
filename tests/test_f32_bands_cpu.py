"""CPU: the band power (include/specan_bands.h: sa_bands_f32 of libspecan_bands.so; SpectrumChain.band_power and
channel_power_f32) as far as no GPU is needed: the numpy mirror frames.bands_of_rows against probes whose expected values
are worked out by hand below (integers, whose sums are exact in any order), never from the code under test; the conditions
under which the order of the header's tree shows in the bits, checked on the inputs the GPU test reuses; the header against
the built library and the binding table abi.BANDS_SIGNATURES; the kernels the six libraries hold; the refusals through
sa_bands_check with made-up addresses (every expected answer follows from the words of the header); the same arithmetic in
a stand-alone program under the host sanitizers.  What it links and its resource remarks: tests/test_reduction_libraries_cpu.py."""
import ctypes
import functools
import itertools
import os

import numpy as np
import pytest

from conftest import N
from kernel_inventory import TABLE, inventory
from native import INCLUDE, compiles_as_c, declared, exported, standalone_checks
from reduction_libraries import BASE, SA_EINVAL, SA_ESHAPE, SA_OK, _shared, built

FAR = BASE + (1 << 40)
FARTHER = BASE + (1 << 41)
HEADER = os.path.join(INCLUDE, "specan_bands.h")
NAMES = ["sa_bands_check", "sa_bands_f32", "sa_bands_last_error", "sa_bands_version"]
FRAC_MAX = 1.0 - 2.0 ** -32
KERNELS = {f"bands_f32_kernel<{f}, {c}>" for f in range(3) for c in ("true", "false")}
# the bands of the order tests: every one wider than 2048 bins
ORDER_BANDS = [(0, N), (100, 16000), (4096, 8193), (1000, 9100), (5, 16379), (8191, 12289)]
AIMED_BAND = (100, 16000)


# ---------------------------------------------------------------------------------------------------------- the test rows
@functools.lru_cache(maxsize=None)
def noise_rows():
    """64 rows of |N(0,1)| noise"""
    return _shared(np.abs(np.random.default_rng(2200).standard_normal((64, N))).astype(np.float32))


@functools.lru_cache(maxsize=None)
def wide_rows():
    """6 rows log-uniform over 12 decades, each with a carrier 1000 times its largest point"""
    rng = np.random.default_rng(2201)
    pts = (10.0 ** rng.uniform(-6.0, 6.0, size=(6, N))).astype(np.float32)
    for r in range(6):
        pts[r, 3000 + 1777 * r] = np.float32(1000.0) * pts[r].max()
    return _shared(pts)


def tree_levels(w):
    """the levels T0..T14 of the header's tree over the float64 rows ``w`` [R, 16384], by the explicit halving: this file's
    own statement of the tree, which the mirror is held against"""
    T = [np.asarray(w, np.float64)]
    while T[-1].shape[1] > 1:
        T.append(T[-1][:, 0::2] + T[-1][:, 1::2])
    assert len(T) == 15
    return T


def tree_prefix(T, r, i):
    """the power the header's descent holds when it stands on leaf i of row r, the leaf included: the left siblings along
    the path from the root, added from the top down, then the leaf"""
    E = np.float64(0.0)
    for l in range(13, -1, -1):
        node = i >> l
        if node & 1:
            E = E + T[l][r, node - 1]
    return E + T[0][r, i]


def banded(v, lo, hi):
    w = np.zeros_like(v)
    w[:, lo:hi] = v[:, lo:hi]
    return w


@functools.lru_cache(maxsize=None)
def aimed_fractions():
    """One fraction per noise row aimed at a bin's own prefix in AIMED_BAND -- ``c[i0] / S`` with c the tree prefix of this
    file -- and the bin: (fracs float64 [64], bins int [64]).  A sequential sum of exact squares of float32 noise runs HIGH
    against the tree on these rows (measured: above the tree prefix at 92 % of the bins, by tens of units in the last place
    from a few thousand bins on), and where it does the first-bin rule lands on the aimed bin like the descent.  So the bin
    of a row is the first of a seeded sequence of bins at which the sequential prefix lies below the tree prefix: there
    the running sum misses t at the aimed bin and the first-bin rule names the next one."""
    pts = noise_rows()
    lo, hi = AIMED_BAND
    v = pts.astype(np.float64) ** 2
    T = tree_levels(banded(v, lo, hi))
    rng = np.random.default_rng(2202)
    bins = np.zeros(64, np.int64)
    for r in range(64):
        seq = np.cumsum(v[r, lo:hi])
        tries = rng.integers(lo + 50, hi - 1000, size=4000)
        bins[r] = next(int(i) for i in tries if seq[i - lo] < tree_prefix(T, r, int(i)))
    fracs = np.array([tree_prefix(T, r, int(bins[r])) / T[14][r, 0] for r in range(64)])
    assert ((fracs > 0.0) & (fracs < FRAC_MAX)).all()
    return _shared(fracs), _shared(bins)


def bands(points, bands_, fracs=(), **kw):
    from fpga_real_time_fft_analyzer_amd import frames
    power, cross = frames.bands_of_rows(points, bands_, fracs, **kw)
    R = points.shape[0]
    assert power.dtype == np.float64 and power.shape == (R, len(bands_)) and power.flags["C_CONTIGUOUS"]
    assert cross.dtype == np.int32 and cross.shape == (R, len(bands_), len(fracs)) and cross.flags["C_CONTIGUOUS"]
    return power, cross


def same_bits(a, b):
    """float64 arrays equal bit for bit, NaNs by position"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint64)[~nan], b.view(np.uint64)[~nan])


# ------------------------------------------------------------------------------------------------------------- the mirror
def test_small_integers_by_hand():
    """Rows of the integers i mod 7 and (3 i) mod 5, some negative: squares and every partial sum are integers far below
    2^53, so any order gives the same double and the descent is the first bin whose running sum reaches t -- both computed
    here in Python integers.  The fractions are dyadic, so t = f S is exact as well."""
    i = np.arange(N)
    ints = np.stack([i % 7, (3 * i) % 5, np.where(i % 3 == 0, -(i % 4), i % 4)]).astype(np.int64)
    pts = ints.astype(np.float32)
    sets = [(0, N), (1, 2), (7, 9), (100, 612), (255, 257), (5000, 16384), (0, 1), (N - 1, N), (1023, 4097)]
    fracs = (0.5, 0.25, 0.0, 0.9375)
    power, cross = bands(pts, sets, fracs)
    for r in range(3):
        sq = [int(x) * int(x) for x in ints[r]]
        for j, (lo, hi) in enumerate(sets):
            S = sum(sq[lo:hi])
            assert power[r, j] == float(S) and S < 2 ** 40, (r, lo, hi)
            for q, f in enumerate(fracs):
                num, den = {0.5: (1, 2), 0.25: (1, 4), 0.0: (0, 1), 0.9375: (15, 16)}[f]
                run, want = 0, None
                for b in range(lo, hi):                           # the first bin with den * running sum >= num * S
                    run += sq[b]
                    if den * run >= num * S:
                        want = b
                        break
                assert cross[r, j, q] == want, (r, lo, hi, f, int(cross[r, j, q]), want)


def test_a_crossing_met_exactly_and_the_plain_cases():
    """A row of ones: the running sum reaches t = 8192 exactly at bin 8191 (>=, not >); an all-zero band and a fraction of 0
    give lo; a single-bin band gives its bin."""
    ones = np.ones((1, N), np.float32)
    power, cross = bands(ones, [(0, N), (100, 612), (77, 78)], (0.5, 0.25, 0.0, 0.5 + 2.0 ** -14))
    assert power[0].tolist() == [16384.0, 512.0, 1.0]
    assert cross[0].tolist() == [[8191, 4095, 0, 8192], [355, 227, 100, 356], [77, 77, 77, 77]]
    zeros = np.zeros((2, N), np.float32)
    zeros[1, 50] = 3.0
    power, cross = bands(zeros, [(0, N), (51, 9000), (50, 51), (0, 51)], (0.0, 0.5, FRAC_MAX))
    assert power.tolist() == [[0.0] * 4, [9.0, 0.0, 9.0, 9.0]]
    assert cross[0].tolist() == [[0] * 3, [51] * 3, [50] * 3, [0] * 3]
    assert cross[1].tolist() == [[0, 50, 50], [51] * 3, [50] * 3, [0, 50, 50]]
    assert not np.signbit(power).any()


def test_specials():
    """-0.0 is +0.0; the float32 denormal 2^-149 is kept and its square is 2^-298; +inf in a band gives an infinite power, the
    crossing of a positive fraction at the inf's bin (inf >= inf) and -1 at fraction 0 (0 inf is a NaN); a NaN inside a band
    gives a NaN and -1, outside it nothing."""
    pts = np.zeros((1, N), np.float32)
    pts[0, 10] = -0.0
    pts[0, 20] = 1e-45
    pts[0, 30] = -2.0
    pts[0, 40] = np.inf
    pts[0, 50] = np.nan
    assert pts.view(np.uint32)[0, 20] == 1 and pts.view(np.uint32)[0, 10] == 0x80000000
    sets = [(10, 11), (20, 21), (0, 25), (0, 31), (25, 45), (0, 45), (45, 55), (0, N), (51, N), (30, 31)]
    power, cross = bands(pts, sets, (0.0, 0.5))
    assert power[0, 0] == 0.0 and not np.signbit(power[0, 0])
    assert power[0, 1] == 2.0 ** -298 == power[0, 2]
    assert power[0, 3] == 4.0 + 2.0 ** -298 == 4.0 and power[0, 9] == 4.0
    assert np.isinf(power[0, 4]) and np.isinf(power[0, 5]) and power[0, 4] > 0
    assert np.isnan(power[0, 6]) and np.isnan(power[0, 7]) and power[0, 8] == 0.0
    assert cross[0].tolist() == [[10, 10], [20, 20], [0, 20], [0, 30], [-1, 40], [-1, 40], [-1, -1], [-1, -1], [51, 51], [30, 30]]
    # the records of field 'power' are not squared; the other float is never looked at
    rec = np.full((1, N, 2), np.nan, np.float32)
    rec[0, :, 1] = 3.0
    rec[0, 7, 1] = 1e-45
    power, cross = bands(rec, [(0, 4), (100, 228), (7, 8)], (0.5,), field="power")
    assert power[0].tolist() == [12.0, 384.0, 2.0 ** -149] and cross[0, :, 0].tolist() == [1, 163, 7]
    rec = np.full((1, N, 2), np.nan, np.float32)
    rec[0, :, 0] = -3.0
    power, cross = bands(rec, [(0, 4), (100, 228)], (0.5,), field="peak")
    assert power[0].tolist() == [36.0, 1152.0] and cross[0, :, 0].tolist() == [1, 163]


def test_bins_outside_a_band_do_not_exist_for_it():
    pts = wide_rows()[:2]
    sets, fracs = [(1000, 3000), (1001, 2999), (1000, 1001), (2999, 3000)], (0.005, 0.5, 0.995)
    p0, c0 = bands(pts, sets, fracs)
    for v in (3e38, np.inf, np.nan, 0.0):
        loud = pts.copy()
        loud[:, 999] = loud[:, 3000] = loud[:, 0] = loud[:, N - 1] = v
        p1, c1 = bands(loud, sets, fracs)
        assert same_bits(p0, p1) and np.array_equal(c0, c1), v
    loud = pts.copy()
    loud[:, 1000] = 3e38
    p1, _ = bands(loud, sets, fracs)
    assert not same_bits(p0[:, 0], p1[:, 0]) and same_bits(p0[:, 1], p1[:, 1])
    # rows are independent, and a band's result does not depend on the other bands of the call
    for r in range(2):
        p1, c1 = bands(pts[r:r + 1], sets[::-1] + sets, fracs[::-1])
        assert same_bits(p1[0, 4:], p0[r]) and same_bits(p1[0, :4], p0[r, ::-1]) and np.array_equal(c1[0, 4:, ::-1], c0[r])


def test_the_tree_is_the_fold_s_tree_continued():
    """A band [64 c, 64 c + 64) is the bucket c of frames.fold_of_mags(x, 1, 64): the float64 s64, bit for bit."""
    from fpga_real_time_fft_analyzer_amd import frames
    for pts in (noise_rows()[:4], wide_rows()):
        s64 = frames.fold_of_mags(pts, 1, 64)[2]
        for cs in (range(0, 16), range(100, 116), range(240, 256)):
            power, _ = bands(pts, [(64 * c, 64 * c + 64) for c in cs])
            assert same_bits(power, s64[:, list(cs)])
    # and the whole tree against this file's own halving
    pts = wide_rows()
    v = pts.astype(np.float64) ** 2
    power, _ = bands(pts, ORDER_BANDS)
    for j, (lo, hi) in enumerate(ORDER_BANDS):
        assert same_bits(power[:, j], tree_levels(banded(v, lo, hi))[14][:, 0])


def test_the_order_shows_in_the_bits():
    """Conditions on the inputs, with the mirror alone: on the noise rows and the wide-range rows a sequential sum
    (np.cumsum) differs from the tree's S in float64 in every row of every band of ORDER_BANDS -- an implementation that
    sums in another order fails the bit compare there -- while rounded to float32 the two agree (printed): the reason the
    output is float64."""
    for name, pts in (("noise", noise_rows()), ("wide", wide_rows())):
        v = pts.astype(np.float64) ** 2
        power, _ = bands(pts, ORDER_BANDS)
        same32 = 0
        for j, (lo, hi) in enumerate(ORDER_BANDS):
            assert hi - lo > 2048
            seq = np.cumsum(v[:, lo:hi], axis=1)[:, -1]
            differ = seq != power[:, j]
            assert differ.all(), (name, lo, hi, np.nonzero(~differ)[0])
            same32 += int((seq.astype(np.float32) == power[:, j].astype(np.float32)).sum())
        print(f"FIGURE {name}: {pts.shape[0]} rows x {len(ORDER_BANDS)} bands differ in float64; equal as float32: {same32} of "
              f"{pts.shape[0] * len(ORDER_BANDS)}")


def test_aimed_fractions_tell_the_descent_from_a_running_sum():
    """One fraction per noise row aimed at a bin's own tree prefix: the rule "first bin whose sequential running sum reaches
    t" names another bin than the mirror's descent in at least half of the 64 rows, so an implementation of that rule fails
    the GPU compare.  The mirror itself lands on the aimed bin or a neighbour."""
    pts = noise_rows()
    lo, hi = AIMED_BAND
    fracs, aimed = aimed_fractions()
    v = pts.astype(np.float64) ** 2
    other = 0
    for r in range(64):
        power, cross = bands(pts[r:r + 1], [AIMED_BAND], (float(fracs[r]),))
        t = fracs[r] * power[0, 0]
        seq = lo + int(np.argmax(np.cumsum(v[r, lo:hi]) >= t))
        other += seq != cross[0, 0, 0]
        assert abs(int(cross[0, 0, 0]) - int(aimed[r])) <= 1, (r, int(cross[0, 0, 0]), int(aimed[r]))
    print(f"FIGURE the sequential rule names another bin in {other} of 64 rows")
    assert other >= 32, other


def test_arguments_of_the_mirror_and_channel_bands():
    from fpga_real_time_fft_analyzer_amd import frames
    assert (frames.BANDS_MAX, frames.BANDS_Q_MAX) == (16, 4)
    pts = noise_rows()[:3]
    p, c = frames.bands_of_rows(pts, [(0, N)])
    assert p.shape == (3, 1) and c.shape == (3, 1, 0) and c.dtype == np.int32
    assert frames.bands_of_rows(np.zeros((0, N), np.float32), [(0, 1), (2, 3)], (0.5,))[1].shape == (0, 2, 1)
    good = dict(bands=[(0, N)], fracs=())
    bad = [dict(bands=[]), dict(bands=[(0, 1)] * 17), dict(bands=[(5, 5)]), dict(bands=[(6, 5)]), dict(bands=[(-1, 5)]),
           dict(bands=[(0, N + 1)]), dict(bands=[(0.0, 5)]), dict(bands=[(0, True)]), dict(bands=[(0, 1, 2)]), dict(bands=[5]),
           dict(bands=5), dict(bands="01"), dict(bands=[(0, 1), "ab"]), dict(fracs=[0.1] * 5), dict(fracs=[-0.1]), dict(fracs=[1.0]),
           dict(fracs=[float("nan")]), dict(fracs=["0.5"]), dict(fracs=[True]), dict(fracs=0.5), dict(fracs=[None]),
           dict(field="mag"), dict(field=0), dict(field=["peak"])]
    for kw in bad:
        with pytest.raises(ValueError):
            frames.bands_of_rows(pts, **dict(good, **kw))
    for wrong in (pts.astype(np.float64), pts[:, :N // 2], pts[0], np.zeros((2, N, 2), np.float32)):
        with pytest.raises(ValueError):
            frames.bands_of_rows(wrong, [(0, N)])
    with pytest.raises(ValueError):
        frames.bands_of_rows(pts, [(0, N)], field="peak")          # records are [R, 16384, 2]
    p2, c2 = frames.bands_of_rows(pts, np.array([[3, 70], [0, N]]), (np.float32(0.5), 0, FRAC_MAX))
    assert p2.shape == (3, 2) and c2.shape == (3, 2, 3) and (c2[:, 1, 2] == N - 1).all() and (c2[:, :, 1] == [3, 0]).all()
    # channel_bands: main, then lower and upper neighbours outwards, clipped
    cb = frames.channel_bands
    assert cb(8192, 200, 250, 1) == [(8092, 8292), (7842, 8042), (8342, 8542)]
    assert cb(8192, 201, 250, 0) == [(8092, 8293)]
    assert cb(100, 300, 300, 2) == [(0, 250), (250, 550), (550, 850)]          # the lower neighbours lie outside
    assert cb(16300, 200, 150, 1) == [(16200, 16384), (16050, 16250), (16350, 16384)]
    assert cb(np.int64(50), np.int32(10), 10, 1) == [(45, 55), (35, 45), (55, 65)]
    for kw in (dict(center=-500, width=100), dict(center=17000, width=100), dict(width=0), dict(spacing=0), dict(adjacent=-1),
               dict(center=1.0), dict(width=True), dict(spacing="3"), dict(adjacent=8)):
        with pytest.raises(ValueError):
            cb(**dict(dict(center=8192, width=100, spacing=100, adjacent=1), **kw))


# ------------------------------------------------------------------------------------------------------------ the surface
@pytest.fixture(scope="module")
def bands_lib():
    return built("bands")


def _c_bands(values):
    from fpga_real_time_fft_analyzer_amd import abi
    return None if values is None else (abi.Band * len(values))(*(abi.Band(lo, hi) for lo, hi in values))


def _c_fracs(values):
    return None if values is None else (ctypes.c_double * len(values))(*values)


@pytest.fixture(scope="module")
def check(bands_lib):
    def call(field=0, a_in=BASE, a_power=FAR, a_cross=FARTHER, rows=3, nb=None, bands=((0, N),), nq=None, fracs=(0.5,)):
        nb = (len(bands) if bands is not None else 1) if nb is None else nb
        nq = (len(fracs) if fracs is not None else 1) if nq is None else nq
        return bands_lib.sa_bands_check(field, a_in, a_power, a_cross, rows, nb, _c_bands(bands), nq, _c_fracs(fracs))
    return call


def test_header_library_and_binding_table(bands_lib):
    """Name for name: declared in specan_bands.h = exported by libspecan_bands.so = bound in abi.BANDS_SIGNATURES; nothing is
    in the other tables or headers, which are what they were."""
    from fpga_real_time_fft_analyzer_amd import abi
    assert declared(HEADER) == NAMES
    assert [n for n in exported(abi.BANDS_LIB_PATH) if "sa_" in n] == NAMES
    assert sorted(abi.BANDS_SIGNATURES) == NAMES
    others = (abi.SIGNATURES, abi.EXT_SIGNATURES, abi.FOLD_SIGNATURES, abi.PEAKS_SIGNATURES, abi.RANK_SIGNATURES, abi.HIST_SIGNATURES)
    assert not set(NAMES) & set().union(*others)
    assert [len(t) for t in others] == [45, 5, 4, 4, 4, 4]
    for other in ("specan.h", "specan_ext.h", "specan_fold.h", "specan_peaks.h", "specan_rank.h", "specan_hist.h"):
        assert not set(NAMES) & set(declared(os.path.join(INCLUDE, other))), other
    for name in NAMES:
        fn, (restype, argtypes) = getattr(bands_lib, name), abi.BANDS_SIGNATURES[name]
        assert fn.argtypes is not None and list(fn.argtypes) == list(argtypes), name
        assert fn.restype is restype is (ctypes.c_char_p if name == "sa_bands_last_error" else ctypes.c_int), name
    assert bands_lib.sa_bands_version() == abi.SA_BANDS_VERSION == 1
    assert (abi.SA_BANDS_MAX, abi.SA_BANDS_Q_MAX) == (16, 4) and ctypes.sizeof(abi.Band) == 8
    text = open(HEADER).read()
    for line in ("#define SA_BANDS_VERSION 1", "#define SA_BANDS_MAX   16", "#define SA_BANDS_Q_MAX 4", "#define SA_BANDS_IN_MAG         0",
                 "#define SA_BANDS_IN_POINT_PEAK  1", "#define SA_BANDS_IN_POINT_POWER 2", "typedef struct { int32_t lo, hi; } sa_band;"):
        assert line in text, line
    assert '#include "specan.h"' in text and "#include \"specan_rank.h\"" not in text
    assert (abi.SA_BANDS_IN_MAG, abi.SA_BANDS_IN_POINT_PEAK, abi.SA_BANDS_IN_POINT_POWER) == (0, 1, 2) == \
        (abi.SA_RANK_IN_MAG, abi.SA_RANK_IN_POINT_PEAK, abi.SA_RANK_IN_POINT_POWER)
    assert bands_lib.sa_bands_last_error() == b""
    assert os.path.basename(abi.BANDS_LIB_PATH) == "libspecan_bands.so"
    assert os.path.dirname(abi.BANDS_LIB_PATH) == os.path.dirname(abi.LIB_PATH)
    assert len(abi.SA_ENTRIES) == 8 and len(abi.SA_EXT_ENTRIES) == 3


def test_header_compiles_as_c99_pedantic(tmp_path):
    compiles_as_c(tmp_path, '#include "specan_bands.h"\n'
                  "int use(const void *p, double *o, int32_t *c, const sa_band *b, const double *f) { return sa_bands_f32(p,"
                  " SA_BANDS_IN_POINT_POWER, o, c, 8, SA_BANDS_MAX, b, SA_BANDS_Q_MAX, f, 0) + sa_bands_check(SA_BANDS_IN_MAG, 16, 32, 64, 0,"
                  " 1, b, 0, f) + sa_bands_version() - SA_BANDS_VERSION + (sa_bands_last_error()[0] != 0) + SA_BANDS_IN_POINT_PEAK - 1"
                  " + (o[0] > 0.0) + b[0].lo + b[0].hi + (int)sizeof(sa_band); }\n")


def test_kernel_inventories(bands_lib):
    """libspecan_bands.so holds the six instantiations, one per input layout with and without crossings, and nothing else;
    the other five libraries hold what they held."""
    from fpga_real_time_fft_analyzer_amd import abi
    assert inventory(abi.BANDS_LIB_PATH) == KERNELS
    for path in (abi.LIB_PATH, abi.FOLD_LIB_PATH, abi.PEAKS_LIB_PATH, abi.RANK_LIB_PATH, abi.HIST_LIB_PATH):
        if not os.path.exists(path):
            abi.build()
    assert inventory(abi.LIB_PATH) == set(TABLE)
    assert inventory(abi.FOLD_LIB_PATH) == {f"fold_mag_f32_kernel<{k}>" for k in range(7)}
    assert inventory(abi.PEAKS_LIB_PATH) == {f"peaks_f32_kernel<{f}>" for f in range(3)}
    assert inventory(abi.RANK_LIB_PATH) == {f"rank_f32_kernel<{f}>" for f in range(3)}
    assert inventory(abi.HIST_LIB_PATH) == {f"hist_f32_kernel<{s}>" for s in range(1, 7)} | {"hist_zero_kernel"}


# -------------------------------------------------------------------------------------------------------------- the check
def sizes(field, rows, nb, nq):
    return rows * 65536 * (2 if field else 1), rows * nb * 8, rows * nb * nq * 4


def test_known_answers_of_the_header(check):
    assert sizes(0, 3, 2, 2) == (196608, 48, 48) and sizes(2, 1, 16, 0) == (131072, 128, 0)
    b2, f2 = ((0, N),) * 2, (0.5,) * 2
    assert check(0, BASE, BASE + 196608, BASE + 196608 + 48, 3, bands=b2, fracs=f2) == SA_OK          # all three touching
    assert check(0, BASE, BASE - 48, BASE - 96, 3, bands=b2, fracs=f2) == SA_OK
    assert check(0, BASE, BASE + 196608 - 8, FAR, 3, bands=b2, fracs=f2) == SA_EINVAL
    assert check(0, BASE, FAR, BASE + 196608 - 4, 3, bands=b2, fracs=f2) == SA_EINVAL
    assert check(0, BASE, BASE + 196608, BASE + 196608 + 44, 3, bands=b2, fracs=f2) == SA_EINVAL      # cross reaches into power
    b16 = ((0, N),) * 16
    assert check(2, BASE, BASE + 131072, 0, 1, bands=b16, fracs=()) == SA_OK
    assert check(2, BASE, BASE + 131072, BASE, 1, bands=b16, fracs=()) == SA_OK                       # no `cross` byte: not looked at
    assert check(2, BASE, BASE + 131072, BASE + 3, 1, bands=b16, fracs=()) == SA_OK
    assert check(2, BASE, BASE + 131072 - 8, 0, 1, bands=b16, fracs=()) == SA_EINVAL
    assert check(2, BASE, BASE - 128, 0, 1, bands=b16, fracs=()) == SA_OK
    assert check(2, BASE, BASE - 120, 0, 1, bands=b16, fracs=()) == SA_EINVAL


def test_touching_and_overlapping_ranges(check):
    """Each of the three pairs: the second range right behind the first and right in front of it is fine; moved into it by
    the smallest step its alignment allows, and by 16 bytes, it is refused; the third range lies far away."""
    X = BASE + (1 << 30)
    for field, rows, nb, nq in itertools.product((0, 1, 2), (1, 5), (1, 3, 16), (1, 4)):
        n = dict(zip(("a_in", "a_power", "a_cross"), sizes(field, rows, nb, nq)))
        step = {"a_in": 16, "a_power": 8, "a_cross": 4}
        away = {"a_in": BASE - (1 << 34), "a_power": FAR, "a_cross": FARTHER}
        kw = dict(field=field, rows=rows, bands=((0, N),) * nb, fracs=(0.5,) * nq)
        for a, b in (("a_in", "a_power"), ("a_in", "a_cross"), ("a_power", "a_cross")):
            third = ({"a_in", "a_power", "a_cross"} - {a, b}).pop()
            tag = (field, rows, nb, nq, a, b)
            at = lambda pa, pb: check(**kw, **{a: pa, b: pb, third: away[third]})      # noqa: E731
            assert at(X, X + n[a]) == SA_OK and at(X, X - n[b]) == SA_OK, tag
            assert at(X, X + n[a] + 16) == SA_OK and at(X, X - n[b] - 16) == SA_OK, tag
            for by in (step[b], 16) if n[a] >= 16 else (step[b],):
                assert at(X, X + n[a] - by) == SA_EINVAL, tag + (by,)
            m = max(step[a], step[b])
            if n[b] > m or n[a] > m:
                assert at(X, X - n[b] + m) == SA_EINVAL, tag
            assert at(X, X) == SA_EINVAL, tag
        for off in (1, 2, 4, 8, 12, 16, 32):
            assert check(**kw, a_in=BASE + off) == (SA_OK if off % 16 == 0 else SA_EINVAL), off
            assert check(**kw, a_power=FAR + off) == (SA_OK if off % 8 == 0 else SA_EINVAL), off
            assert check(**kw, a_cross=FARTHER + off) == (SA_OK if off % 4 == 0 else SA_EINVAL), off
        for null in ("a_in", "a_power", "a_cross"):
            assert check(**kw, **{null: 0}) == SA_EINVAL, null
    # with nq 0, `cross` is never looked at: NULL, misaligned, inside `in`
    for a_cross in (0, 3, BASE, BASE + 5, FAR):
        assert check(fracs=(), a_cross=a_cross) == SA_OK, a_cross


def test_refusals_in_their_order(check, bands_lib):
    """1 negative rows, 2 the scalar arguments, the bands and the fractions (also at rows 0), 3 the empty call, 4 the
    pointers: each refusal is shown to win over every later one by making the later ones wrong too."""
    bad = [dict(field=-1), dict(field=3), dict(nb=0), dict(nb=17), dict(nb=-1), dict(bands=None), dict(bands=((5, 5),)),
           dict(bands=((6, 5),)), dict(bands=((-1, 5),)), dict(bands=((0, N + 1),)), dict(bands=((N, N + 1),)),
           dict(bands=((0, N),) * 15 + ((7, 7),)), dict(bands=((-2 ** 31, 2 ** 31 - 1),)), dict(nq=-1), dict(nq=5), dict(fracs=None),
           dict(fracs=(1.0,)), dict(fracs=(-1e-300,)), dict(fracs=(float("nan"),)), dict(fracs=(0.5, 0.5, 0.5, 2.0)),
           dict(fracs=(float("inf"),)), dict(fracs=(np.nextafter(FRAC_MAX, 2.0),))]
    wrong_ptrs = [dict(), dict(a_in=0, a_power=0, a_cross=0), dict(a_in=BASE + 1, a_power=BASE + 3, a_cross=BASE + 2),
                  dict(a_in=BASE, a_power=BASE, a_cross=BASE)]
    # 1: before bad arguments and bad pointers
    for kw in [dict()] + bad:
        for p in wrong_ptrs:
            assert check(rows=-1, **kw, **p) == SA_ESHAPE, (kw, p)
            assert check(rows=-(1 << 31), **kw, **p) == SA_ESHAPE, (kw, p)
    # 2: before the empty call and the pointers
    for rows in (0, 1, 5, (1 << 31) - 1):
        for kw in bad:
            for p in wrong_ptrs:
                assert check(rows=rows, **kw, **p) == SA_EINVAL, (rows, kw, p)
    # 3: the empty call is SA_OK whatever the pointers are
    for p in wrong_ptrs:
        for field in (0, 1, 2):
            assert check(field=field, rows=0, **p) == SA_OK, p
    # 4: the pointers, last
    for p in wrong_ptrs[1:]:
        assert check(rows=1, **p) == SA_EINVAL, p
    assert check(rows=1) == SA_OK
    # within 2: the counts are judged before the arrays are read -- the call returns at all with nb = 17 and an array of one
    # band, nq = 5 and one fraction (the stand-alone program holds every array at exactly its count under the address
    # sanitizer)
    assert check(nb=17, bands=((0, N),)) == SA_EINVAL and check(nq=5, fracs=(0.5,)) == SA_EINVAL
    assert check(nb=0, bands=None) == SA_EINVAL and check(nq=0, fracs=None) == SA_OK
    # the edges of every scalar that are good
    for kw in (dict(bands=((0, 1),)), dict(bands=((N - 1, N),) * 16), dict(fracs=(0.0,)), dict(fracs=(FRAC_MAX,) * 4), dict(fracs=()),
               dict(field=2), dict(bands=((5, 9), (0, N), (5, 9))), dict(fracs=(0.995, 0.005)),
               dict(rows=(1 << 31) - 1, a_in=1 << 20, a_power=1 << 62, a_cross=1 << 63)):
        assert check(**kw) == SA_OK, kw
    assert bands_lib.sa_bands_last_error() == b""                 # the check alone leaves the thread's text alone


def test_standalone_program_under_host_sanitizers(tmp_path):
    """tests/cpp/test_sa_bands_check.cpp + csrc/sa_bands_check.cpp, host only, under the address and undefined-behaviour
    sanitizers when they link here (a plain build otherwise: the program's own checks still run): the same arithmetic at rows
    up to 2^31 - 1 and addresses near 2^47 and 2^64, every array of bands and fractions exactly as long as its count.
    Nothing is loaded into this process."""
    assert standalone_checks(tmp_path, "test_sa_bands_check", ["sa_bands_check.cpp"]) > 100000


# ----------------------------------------------------------------------------------------------------------- the wrappers
def test_the_wrappers_surface():
    """The Python entry points exist with the signatures of the issue; a bad band set, fraction, field or group is SA_EINVAL
    before anything of the object or of a library is touched (the object here has neither)."""
    import inspect

    from fpga_real_time_fft_analyzer_amd import chain
    cls = chain.SpectrumChain
    assert list(inspect.signature(cls.band_power).parameters) == ["self", "t", "bands", "fracs", "field", "power", "cross"]
    assert list(inspect.signature(cls.channel_power_f32).parameters) == ["self", "x", "bands", "fracs", "group", "scale", "work",
                                                                         "power", "cross"]
    assert inspect.signature(cls.channel_power_f32).parameters["scale"].default == 1.0 / 2048.0
    assert inspect.signature(cls.band_power).parameters["fracs"].default == ()
    bare = object.__new__(cls)
    bad = [dict(bands=[]), dict(bands=[(0, 1)] * 17), dict(bands=[(5, 5)]), dict(bands=[(0, N + 1)]), dict(bands=[(-1, 4)]),
           dict(bands=[(0.0, 4)]), dict(bands=[(0, True)]), dict(bands=None), dict(bands=7), dict(bands="ab"), dict(bands=[(1, 2, 3)]),
           dict(fracs=[0.5] * 5), dict(fracs=[1.0]), dict(fracs=[-0.5]), dict(fracs=[float("nan")]), dict(fracs=["0.5"]),
           dict(fracs=0.5), dict(fracs=[True]), dict(field="mag"), dict(field=0), dict(field=["peak"])]
    for kw in bad:
        with pytest.raises(chain.SpecanError) as e:
            bare.band_power(None, **dict(dict(bands=[(0, N)]), **kw))
        assert e.value.code == SA_EINVAL and "tensor" not in str(e.value), (kw, str(e.value))
        if "field" not in kw:
            with pytest.raises(chain.SpecanError) as e:
                bare.channel_power_f32(None, **dict(dict(bands=[(0, N)]), **kw))
            assert e.value.code == SA_EINVAL and "tensor" not in str(e.value), (kw, str(e.value))
    for group in (0, 1, 3, 256, 2.0, True, "4"):
        with pytest.raises(chain.SpecanError) as e:
            bare.channel_power_f32(None, [(0, N)], group=group)
        assert e.value.code == SA_EINVAL, group
        assert ("group" in str(e.value) or "folds nothing" in str(e.value)) and "tensor" not in str(e.value), (group, str(e.value))
    with pytest.raises(chain.SpecanError) as e:                   # with good arguments the input's check does speak
        bare.channel_power_f32(None, [(0, N)], (0.005, 0.995), group=4)
    assert e.value.code == SA_EINVAL and "tensor" in str(e.value)
    assert cls._bands_args([(np.int64(1), 5), (0, N)], (0, np.float32(0.5)), "power") == (2, ((1, 5), (0, N)), (0.0, 0.5))
    assert cls._bands_args(((3, 4),), (), None) == (0, ((3, 4),), ()) and cls._bands_args([[3, 4]], [FRAC_MAX], "peak")[0] == 1
    assert not [n for n in dir(chain) if n.endswith("_CHAIN") and "BAND" in n]
    assert set(chain.reductions.FIELDS) == {None, "peak", "power"}
