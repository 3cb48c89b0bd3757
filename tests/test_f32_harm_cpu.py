"""CPU: the harmonic analysis (include/specan_harm.h: sa_harm_f32 of libspecan_harm.so) without a GPU -- the numpy mirror
frames.harm_of_rows on planted spectra, by hand on the alias table, against frames.bands_of_rows and on edge rows;
frames.harm_metrics; the header against the library's exports and the binding table; the argument check as a pure function
and as a stand-alone program under the host sanitizers.  What it links and its resource remarks: tests/test_reduction_libraries_cpu.py.

The rows made here are the data of tests/test_gpu_f32_harm.py too, which holds the device against the mirror bit for bit."""
import ctypes
import functools
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

HEADER = os.path.join(INCLUDE, "specan_harm.h")
NAMES = ["sa_harm_check", "sa_harm_f32", "sa_harm_last_error", "sa_harm_version"]
KERNELS = {f"harm_f32_kernel<{f}>" for f in range(3)}
HALF = N // 2
PLANTED_AMPS = (1e-3, 3e-4, 1e-4, 5e-5)                          # harmonics 2..5 against a fundamental of 1
SUMS = ("dist", "nad", "noise")
WORDS = ("bin", "fund", "spur", "nonharm", "spur_bin", "nonharm_bin", "n_noise")


def harm(pts, field=None, **kw):
    from fpga_real_time_fft_analyzer_amd import frames
    return frames.harm_of_rows(records_of(pts, field), field=field, **kw)


def same_records(a, b):
    """None where two HARM_ROW arrays are equal bit for bit (a NaN sum by position, the floats as words), else what differs"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return f"{a.dtype} {a.shape} against {b.dtype} {b.shape}"
    for name in ("power",) + SUMS:
        if not same_bits(a[name], b[name]):
            return f"{name}: rows {np.argwhere(np.atleast_2d(a[name].T != b[name].T).any(axis=0)).ravel()[:5].tolist()}"
    for name in WORDS:
        x, y = np.ascontiguousarray(a[name]).view(np.int32), np.ascontiguousarray(b[name]).view(np.int32)
        if not np.array_equal(x, y):
            return f"{name}: rows {np.argwhere((x != y).reshape(len(a), -1).any(axis=1)).ravel()[:5].tolist()}"
    return None


@functools.lru_cache(maxsize=None)
def planted():
    """[2, N] float32: the magnitudes of numpy.fft.fft of a Hann-windowed float64 frame holding a coherent tone at bin 1001
    and at bin 6001 with harmonics 2..5 of the amplitudes PLANTED_AMPS"""
    n = np.arange(N)
    rows = []
    for k1 in (1001, 6001):
        x = np.cos(2 * np.pi * k1 * n / N)
        for h, a in zip(range(2, 6), PLANTED_AMPS):
            x = x + a * np.cos(2 * np.pi * ((h * k1) % N) * n / N + 0.3 * h)
        rows.append(np.abs(np.fft.fft(x * (0.5 - 0.5 * np.cos(2 * np.pi * n / N)))))
    return _shared(np.stack(rows).astype(np.float32))


def plant(rng, k1, rows, floor=1.0, peak=1000.0):
    """``rows`` rows of a random float32 floor in (0, floor) with the maximum of bins 0..8192 planted at bin ``k1`` and a
    larger point still above 8192, which no analysis may see"""
    pts = (floor * rng.random((rows, N))).astype(np.float32)
    pts[:, k1] = np.float32(peak) * (1 + np.arange(rows, dtype=np.float32))
    pts[:, 9000 + k1 // 2] = np.float32(1e6)
    return pts


def brute(row, order, span, lo, hi, fund, dc, top, power_field=False):
    """One row by the words of the header, with Python sets of bins and the explicit halving: a dict of the record"""
    bits = row.view(np.uint32) & np.uint32(0x7FFFFFFF)
    a = bits.view(np.float32).astype(np.float64)
    v = a if power_field else a * a
    keys = [int(b) for b in bits]
    k1 = fund if fund >= 0 else max(range(lo, hi), key=lambda i: (keys[i], -i))
    ks = []
    for h in range(1, order + 1):
        m = (h * k1) % N
        ks.append(m if m <= HALF else N - m)
    band = [set(range(max(k - span, dc), min(k + span + 1, top))) for k in ks]
    F = band[0]
    B = [b - F for b in band[1:]]
    U = set().union(*B) if B else set()
    A = set(range(dc, top))

    def tree(members):
        w = np.zeros(N, np.float64)
        at = sorted(members)
        w[at] = v[at]
        while len(w) > 1:
            w = w[0::2] + w[1::2]
        return w[0]

    def largest(members):
        if not members:
            return 0, -1
        at = max(sorted(members), key=lambda i: (keys[i], -i))
        return keys[at], at

    with np.errstate(over="ignore", invalid="ignore"):
        out = dict(power=[tree(F)] + [tree(b) for b in B] + [0.0] * (10 - order), dist=tree(U), nad=tree(A - F), noise=tree(A - F - U))
    out["bin"] = ks + [-1] * (10 - order)
    out["fund"] = keys[k1]
    out["spur"], out["spur_bin"] = largest(A - F)
    out["nonharm"], out["nonharm_bin"] = largest(A - F - U)
    out["n_noise"] = len(A - F - U)
    return out


def assert_brute(pts, tag, field=None, **kw):
    from fpga_real_time_fft_analyzer_amd import frames
    dc, top, lo, hi, fund, span, order = frames._harm_args(kw.get("order", 5), kw.get("span", 3), kw.get("lo"), kw.get("hi"),
                                                            kw.get("fund"), kw.get("dc"), kw.get("top", HALF + 1), field)
    rec = harm(pts, field, **kw)
    for r in range(len(pts)):
        want = brute(pts[r], order, span, lo, hi, fund, dc, top, field == "power")
        assert same_bits(rec["power"][r], np.array(want["power"])), (tag, r, "power")
        for name in SUMS:
            assert same_bits(rec[name][r], np.float64(want[name])), (tag, r, name)
        assert rec["bin"][r].tolist() == want["bin"], (tag, r)
        for name in ("fund", "spur", "nonharm"):
            assert int(rec[name][r:r + 1].view(np.uint32)[0]) == want[name], (tag, r, name)
        for name in ("spur_bin", "nonharm_bin", "n_noise"):
            assert int(rec[name][r]) == want[name], (tag, r, name)
    return rec


# ------------------------------------------------------------------------------------------------------------- the mirror
def test_planted_tones_give_the_planted_ratios():
    """hd_dbc and thd_dbc equal the planted ratios to 1e-3 dB (the float32 rounding of the magnitudes bounds the error near
    1e-6 dB: a Hann window spreads every coherent tone over the same three bins, so the ratio of two band powers is the ratio
    of the squared amplitudes); the worst spur is the second harmonic; 6001 folds to 4382, 1619, 7620, 2763."""
    from fpga_real_time_fft_analyzer_amd import frames
    rec = harm(planted(), order=5, span=3)
    assert rec.dtype == frames.HARM_ROW and rec.shape == (2,)
    assert rec["bin"][0].tolist() == [1001, 2002, 3003, 4004, 5005] + [-1] * 5
    assert rec["bin"][1].tolist() == [6001, 4382, 1619, 7620, 2763] + [-1] * 5
    m = frames.harm_metrics(rec)
    want_hd = 20 * np.log10(np.array(PLANTED_AMPS))
    want_thd = 10 * np.log10(sum(a * a for a in PLANTED_AMPS))
    for r in range(2):
        err = np.abs(m["hd_dbc"][r, 1:5] - want_hd)
        print("FIGURE hd error dB", err.tolist(), "thd error dB", abs(m["thd_dbc"][r] - want_thd))
        assert (err <= 1e-3).all() and abs(m["thd_dbc"][r] - want_thd) <= 1e-3
        assert m["hd_dbc"][r, 0] == 0.0 and np.isnan(m["hd_dbc"][r, 5:]).all()
        assert rec["spur_bin"][r] == rec["bin"][r, 1]
        assert abs(m["sfdr_dbc"][r] - 60.0) <= 1e-3
        assert abs(m["sinad_db"][r] + m["thd_dbc"][r]) <= 1e-3 and m["snr_db"][r] > 150.0     # no noise but the rounding
        assert m["enob"][r] == (m["sinad_db"][r] - 1.76) / 6.02
        assert rec["n_noise"][r] == HALF + 1 - 4 - 5 * 7 and rec["nonharm_bin"][r] not in rec["bin"][r]
    assert same_records(rec[:1], harm(planted()[:1])) is None
    # the power unit: the same rows squared, as records
    sq = (planted().astype(np.float64) ** 2).astype(np.float32)
    mp = frames.harm_metrics(harm(sq, "power"), unit="power")
    assert np.abs(mp["sfdr_dbc"] - 60.0).max() <= 1e-3 and np.abs(mp["hd_dbc"][:, 1:5] - want_hd).max() <= 1e-3
    with pytest.raises(ValueError):
        frames.harm_metrics(rec, unit="dB")
    with pytest.raises(ValueError):
        frames.harm_metrics(np.zeros(2))


def test_alias_table_by_hand():
    from fpga_real_time_fft_analyzer_amd import frames
    assert frames.harm_alias_bins(2731, 5).tolist() == [2731, 5462, 8191, 5460, 2729]
    assert frames.harm_alias_bins(4096, 5).tolist() == [4096, 8192, 4096, 0, 4096]
    assert frames.harm_alias_bins(8192, 10).tolist() == [8192, 0] * 5
    assert frames.harm_alias_bins(6001, 5).tolist() == [6001, 4382, 1619, 7620, 2763]
    assert frames.harm_alias_bins(5461, 4).tolist() == [5461, 5462, 1, 5460]
    assert frames.harm_alias_bins([3, 0], 10).tolist() == [[3 * h for h in range(1, 11)], [0] * 10]
    rng = np.random.default_rng(2401)
    for k1, want in ((2731, [2731, 5462, 8191, 5460, 2729]), (4096, [4096, 8192, 4096, 0, 4096]), (8192, [8192, 0, 8192, 0, 8192])):
        pts = plant(rng, k1, 2)
        rec = assert_brute(pts, k1)
        assert rec["bin"][:, :5].tolist() == [want] * 2
        if k1 == 4096:                                            # harmonics 3 and 5 lie on the fundamental, 4 below dc
            assert (rec["power"][:, 2:] == 0.0).all() and not np.signbit(rec["power"][:, 2:]).any() and (rec["power"][:, :2] > 0).all()
            assert (rec["dist"] == rec["power"][:, 1]).all()
        if k1 == 8192:                                            # the band is cut by top; the even harmonics fall below dc
            assert (rec["power"][:, 1:] == 0.0).all() and (rec["dist"] == 0.0).all() and (rec["n_noise"] == HALF + 1 - 4 - 4).all()


def test_power_slots_against_band_power():
    """power[0] is bands_of_rows of the band F bit for bit, and power[h - 1] that of harmonic h's band wherever it does not
    meet F; dist, nad and noise are trees of their own: on noise rows nad differs from noise + dist in the last bits."""
    from fpga_real_time_fft_analyzer_amd import frames
    pts = noise_rows()[:6].copy()
    for r, k1 in enumerate((1001, 6001, 255, 2731, 4096, 700)):
        pts[r, k1] = 50.0
    for span in (0, 3, 64):
        rec = harm(pts, order=10, span=span)
        dc, top = span + 1, HALF + 1
        differs = 0
        for r in range(6):
            f = (max(rec["bin"][r, 0] - span, dc), min(rec["bin"][r, 0] + span + 1, top))
            ranges = [(max(k - span, dc), min(k + span + 1, top)) for k in rec["bin"][r]]
            for h, (lo, hi) in enumerate(ranges):
                if lo >= hi:
                    assert rec["power"][r, h] == 0.0
                elif h == 0 or hi <= f[0] or lo >= f[1]:
                    want, _ = frames.bands_of_rows(pts[r:r + 1], [(lo, hi)])
                    assert same_bits(rec["power"][r, h], want[0, 0]), (span, r, h)
            want, _ = frames.bands_of_rows(pts[r:r + 1], [(dc, top), f])
            assert abs(rec["nad"][r] - (want[0, 0] - want[0, 1])) <= 1e-12 * want[0, 0]
            differs += rec["nad"][r] != rec["noise"][r] + rec["dist"][r]
        assert span == 0 or differs > 0


def test_edge_rows():
    from fpga_real_time_fft_analyzer_amd import frames
    rng = np.random.default_rng(2402)
    # ties go to the lowest bin: the fundamental, the spur and the non-harmonic spur
    pts = (0.5 * rng.random((3, N))).astype(np.float32)
    pts[0, [700, 5000, 7000]] = 9.0                               # three equal maxima
    pts[1, [700, 5000]] = -9.0                                    # the sign is cleared
    pts[1, [300, 6000]] = 4.0
    pts[2, 100] = 9.0
    pts[2, [200, 201, 8000]] = 4.0                                # 200 is the second harmonic: the non-harmonic tie is 201 | 8000
    rec = assert_brute(pts, "ties", order=3, span=0)
    assert rec["bin"][:, 0].tolist() == [700, 700, 100] and rec["spur_bin"].tolist() == [5000, 5000, 200]
    assert rec["nonharm_bin"].tolist() == [5000, 5000, 201] and rec["fund"].tolist() == [9.0] * 3
    assert harm(pts, order=3, span=0, lo=701)["bin"][:2, 0].tolist() == [5000, 5000]
    # an all-zero row (and one of -0.0): k1 = lo, spur +0.0 at the first analysed bin outside F
    zero = np.zeros((2, N), np.float32)
    zero[1] = -0.0
    rec = assert_brute(zero, "zero", order=5, span=3)
    assert rec["bin"][:, 0].tolist() == [4, 4] and rec["spur_bin"].tolist() == [8, 8] and rec["nonharm_bin"].tolist() == [24, 24]
    assert rec["n_noise"].tolist() == [HALF + 1 - 24] * 2      # F = [4, 8), the harmonics at 8, 12, 16, 20 cover [8, 24)
    assert (rec["spur"].view(np.uint32) == 0).all()
    assert (rec["power"] == 0).all() and not np.signbit(rec["power"]).any() and not np.signbit(rec["nad"]).any()
    rec = assert_brute(zero[:1], "zero, lo", order=2, span=3, lo=1000, hi=1001, dc=0)
    assert rec["bin"][0, :2].tolist() == [1000, 2000] and rec["spur_bin"][0] == 0
    # a NaN is the fundamental, and the sums it is in are NaNs
    pts = plant(rng, 1500, 3)
    pts[1, 2222] = np.nan
    pts[2, 9999] = np.nan                                         # above the analysed bins: it does not exist
    rec = assert_brute(pts, "nan", order=4, span=2)
    assert rec["bin"][:, 0].tolist() == [1500, 2222, 1500] and np.isnan(rec["fund"][1]) and np.isnan(rec["power"][1, 0])
    assert not np.isnan(rec["nad"][1]) and not np.isnan(rec["power"][2]).any()
    clean = pts[2:].copy()
    clean[0, 9999] = 0.0
    assert same_records(rec[2:], harm(clean, order=4, span=2)) is None
    rec = assert_brute(pts, "nan, fund", order=4, span=2, fund=1500)
    assert np.isnan(rec["spur"][1]) and rec["spur_bin"][1] == 2222 and np.isnan(rec["noise"][1]) and np.isnan(rec["nad"][1])
    assert not np.isnan(rec["power"][1]).any() and not np.isnan(rec["dist"][1])
    # +inf, denormals
    pts = plant(rng, 3000, 2, floor=1e-45 * 4)
    pts[1, 6000] = np.inf
    rec = assert_brute(pts, "inf", order=3, span=1)
    assert rec["bin"][1, 0] == 6000 and np.isinf(rec["power"][1, 0]) and rec["noise"][0] > 0 and rec["noise"][0] < 1e-80
    # order 1, span 0 and 64, top below the harmonics, fund given against fund searched
    pts = plant(rng, 1234, 2)
    rec = assert_brute(pts, "order 1", order=1, span=3)
    assert (rec["bin"][:, 1:] == -1).all() and (rec["dist"] == 0).all() and same_bits(rec["nad"], rec["noise"])
    assert (rec["nonharm_bin"] == rec["spur_bin"]).all()
    assert_brute(pts, "span 0", order=10, span=0)
    assert_brute(pts, "span 64", order=10, span=64)
    assert_brute(pts, "span 64, dc 0", order=10, span=64, dc=0)
    rec = assert_brute(pts, "top 4000", order=10, span=2, top=4000)
    assert rec["bin"][0].tolist() == [1234, 2468, 3702, 4936, 6170, 7404, 7746, 6512, 5278, 4044]
    assert (rec["power"][:, 3:] == 0).all() and (rec["power"][:, :3] > 0).all()
    assert same_records(harm(pts, order=10, span=2), harm(pts, order=10, span=2, fund=1234)) is None
    assert same_records(harm(pts, order=10, span=2), harm(pts, order=10, span=2, fund=-1)) is None
    other = assert_brute(pts, "fund 1000", order=10, span=2, fund=1000)
    assert other["bin"][0, :3].tolist() == [1000, 2000, 3000] and other["spur_bin"].tolist() == [1234, 1234]
    # F is all there is: both largest are (+0.0, -1)
    rec = assert_brute(pts, "only F", order=2, span=64, dc=1200, top=1260)
    assert rec["spur_bin"].tolist() == [-1, -1] and rec["nonharm_bin"].tolist() == [-1, -1] and (rec["n_noise"] == 0).all()


@pytest.mark.parametrize("field", FIELDS)
def test_fields_and_boundary_fundamentals(field):
    """every fundamental of the GPU file's list once by brute force, in every layout"""
    rng = np.random.default_rng(2403)
    for k1, span, top in ((3, 2, HALF + 1), (255, 64, HALF + 1), (1024, 0, HALF + 1), (5461, 2, 4000) if field else (8191, 64, HALF + 1)):
        k1 = min(k1, top - 1)
        pts = plant(rng, k1, 1)
        rec = assert_brute(pts, (field, k1), field=field, order=10, span=span, top=top, dc=0 if k1 == 3 else None)
        assert rec["bin"][0, 0] == k1


def test_arguments_of_the_mirror():
    from fpga_real_time_fft_analyzer_amd import frames
    pts = np.zeros((1, N), np.float32)
    assert frames._harm_args(5, 3, None, None, None, None, 8193, None) == (4, 8193, 4, 8193, -1, 3, 5)
    assert frames._harm_args(np.int64(10), 64, 70, 71, 70, 0, 100, "power") == (0, 100, 70, 71, 70, 64, 10)
    bad = [dict(order=0), dict(order=11), dict(order=5.0), dict(order=True), dict(order=None), dict(span=-1), dict(span=65),
           dict(span="3"), dict(span=None), dict(top=8194), dict(top=4), dict(top=None), dict(top=0), dict(dc=-1), dict(dc=8193),
           dict(dc=1.0), dict(lo=3), dict(lo=8193), dict(hi=8194), dict(lo=100, hi=100), dict(lo=101, hi=100), dict(hi=False),
           dict(fund=3), dict(fund=8193), dict(fund=-2), dict(fund=7.0), dict(dc=10, fund=9), dict(top=100, fund=100),
           dict(top=100, hi=101), dict(field="mag"), dict(field=0), dict(field=["peak"])]
    for kw in bad:
        with pytest.raises(ValueError):
            frames.harm_of_rows(pts, **kw)
    for wrong in (pts.astype(np.float64), pts[0], np.zeros((1, N, 2), np.float32), np.zeros((1, N - 1), np.float32)):
        with pytest.raises(ValueError):
            frames.harm_of_rows(wrong)
    with pytest.raises(ValueError):
        frames.harm_of_rows(pts, field="peak")
    assert frames.harm_of_rows(np.zeros((0, N), np.float32)).shape == (0,)
    assert frames.harm_of_rows(np.zeros((1, N, 2), np.float32), field="power", fund=8192, span=0, order=1)["bin"][0, 0] == 8192


# ------------------------------------------------------------------------------------------------------------ the surface
@pytest.fixture(scope="module")
def harm_lib():
    return built("harm")


GOOD = dict(dc=4, top=8193, lo=4, hi=8193, fund=-1, span=3, order=5)


@pytest.fixture(scope="module")
def check(harm_lib):
    from fpga_real_time_fft_analyzer_amd import abi

    def call(field=0, rows=3, cfg=True, **kw):
        addr = {"in": kw.pop("in", BASE), "out": kw.pop("out", BASE + (1 << 40))}
        c = abi.HarmCfg(**dict(GOOD, **kw)) if cfg else None
        return harm_lib.sa_harm_check(field, addr["in"], addr["out"], rows, ctypes.byref(c) if cfg else None)
    return call


def test_header_library_and_binding_table(harm_lib):
    """Name for name: declared in specan_harm.h = exported by libspecan_harm.so = bound in abi.HARM_SIGNATURES; nothing is in
    the other tables or headers, which are what they were.  The record three times: the header's struct, the binding's
    Structure, the mirror's dtype."""
    from fpga_real_time_fft_analyzer_amd import abi, frames
    assert declared(HEADER) == NAMES
    assert [n for n in exported(abi.HARM_LIB_PATH) if "sa_" in n] == NAMES
    assert sorted(abi.HARM_SIGNATURES) == NAMES
    others = (abi.SIGNATURES, abi.EXT_SIGNATURES, abi.FOLD_SIGNATURES, abi.PEAKS_SIGNATURES, abi.RANK_SIGNATURES, abi.HIST_SIGNATURES,
              abi.BANDS_SIGNATURES, abi.MASK_SIGNATURES)
    assert not set(NAMES) & set().union(*others)
    assert [len(t) for t in others] == [45, 5, 4, 4, 4, 4, 4, 4]
    for other in ("specan.h", "specan_ext.h", "specan_fold.h", "specan_peaks.h", "specan_rank.h", "specan_hist.h", "specan_bands.h",
                  "specan_mask.h"):
        assert not set(NAMES) & set(declared(os.path.join(INCLUDE, other))), other
    for name in NAMES:
        fn, (restype, argtypes) = getattr(harm_lib, name), abi.HARM_SIGNATURES[name]
        assert fn.argtypes is not None and list(fn.argtypes) == list(argtypes), name
        assert fn.restype is restype is (ctypes.c_char_p if name == "sa_harm_last_error" else ctypes.c_int), name
    assert harm_lib.sa_harm_version() == abi.SA_HARM_VERSION == 1
    text = open(HEADER).read()
    for line in ("#define SA_HARM_VERSION 1", "#define SA_HARM_MAX      10", "#define SA_HARM_SPAN_MAX 64", "#define SA_HARM_TOP_MAX  8193",
                 "#define SA_HARM_IN_MAG         0", "#define SA_HARM_IN_POINT_PEAK  1", "#define SA_HARM_IN_POINT_POWER 2",
                 "int sa_harm_f32(const void *in, int field, sa_harm_row *out, int rows, const sa_harm_cfg *cfg, void *stream);"):
        assert line in text, line
    assert '#include "specan.h"' in text and "#include \"specan_bands.h\"" not in text
    assert (abi.SA_HARM_IN_MAG, abi.SA_HARM_IN_POINT_PEAK, abi.SA_HARM_IN_POINT_POWER) == (0, 1, 2) == \
        (abi.SA_BANDS_IN_MAG, abi.SA_BANDS_IN_POINT_PEAK, abi.SA_BANDS_IN_POINT_POWER)
    assert (abi.SA_HARM_MAX, abi.SA_HARM_SPAN_MAX, abi.SA_HARM_TOP_MAX) == (10, 64, 8193) == \
        (frames.HARM_MAX, frames.HARM_SPAN_MAX, frames.HARM_TOP_MAX)
    assert ctypes.sizeof(abi.HarmRow) == 168 == frames.HARM_ROW.itemsize and ctypes.sizeof(abi.HarmCfg) == 28
    assert [n for n, _ in abi.HarmRow._fields_] == list(frames.HARM_ROW.names)
    offsets = [getattr(abi.HarmRow, n).offset for n, _ in abi.HarmRow._fields_]
    assert offsets == [frames.HARM_ROW.fields[n][1] for n in frames.HARM_ROW.names] == [0, 80, 88, 96, 104, 144, 148, 152, 156, 160, 164]
    # the header's two structs, member for member in the order of the binding
    struct = re.search(r"typedef struct \{([^}]*)\} sa_harm_row;", re.sub(r"/\*.*?\*/", "", text, flags=re.S)).group(1)
    assert re.findall(r"\b([a-z_]+)(?:\[SA_HARM_MAX\])?[,;]", struct) == list(frames.HARM_ROW.names)
    assert re.findall(r"(double|int32_t|float)\s", struct) == ["double", "double", "int32_t", "float", "int32_t"]
    struct = re.search(r"typedef struct \{([^}]*)\} sa_harm_cfg;", text).group(1)
    assert re.findall(r"\b([a-z]+)[,;]", struct) == [n for n, _ in abi.HarmCfg._fields_] == list(GOOD)
    assert set(re.findall(r"(double|int32_t|float)\s", struct)) == {"int32_t"}
    assert harm_lib.sa_harm_last_error() == b""
    assert os.path.basename(abi.HARM_LIB_PATH) == "libspecan_harm.so"
    assert os.path.dirname(abi.HARM_LIB_PATH) == os.path.dirname(abi.LIB_PATH)


def test_header_compiles_as_c99_pedantic(tmp_path):
    compiles_as_c(tmp_path, '#include "specan_harm.h"\n'
                  "int use(const void *p, sa_harm_row *o) { sa_harm_cfg c = {4, SA_HARM_TOP_MAX, 4, 8193, -1, 3, SA_HARM_MAX};"
                  " return sa_harm_f32(p, SA_HARM_IN_POINT_POWER, o, 8, &c, 0) + sa_harm_check(SA_HARM_IN_MAG, 16, 1 << 20, 1, &c)"
                  " + sa_harm_version() - SA_HARM_VERSION + (sa_harm_last_error()[0] != 0) + SA_HARM_IN_POINT_PEAK - 1"
                  " + (o[0].power[9] > o[0].dist) + (o[0].nad > o[0].noise) + o[0].bin[9] + (o[0].fund > o[0].spur)"
                  " + (o[0].nonharm > 0) + o[0].spur_bin + o[0].nonharm_bin + o[0].n_noise + c.span + SA_HARM_SPAN_MAX"
                  " + (int)sizeof(sa_harm_row); }\n")


def test_kernel_inventory(harm_lib):
    """libspecan_harm.so holds the three instantiations, one per input layout, and nothing else."""
    from fpga_real_time_fft_analyzer_amd import abi
    assert inventory(abi.HARM_LIB_PATH) == KERNELS


# -------------------------------------------------------------------------------------------------------------- the check
def sizes(field, rows):
    return {"in": rows * 65536 * (2 if field else 1), "out": rows * 168}


def test_known_answers_of_the_header(check):
    assert list(sizes(0, 3).values()) == [196608, 504] and list(sizes(2, 1).values()) == [131072, 168]
    assert check(0, **{"in": BASE, "out": BASE + 196608}) == SA_OK                   # touching, in a row
    assert check(0, **{"in": BASE, "out": BASE + 196608 - 8}) == SA_EINVAL
    assert check(1, **{"in": BASE, "out": BASE + 196608}) == SA_EINVAL               # records read twice as much
    assert check(0, **{"in": BASE, "out": BASE - 504}) == SA_OK
    assert check(0, **{"in": BASE, "out": BASE - 496}) == SA_EINVAL
    assert check(2, rows=1, **{"in": BASE, "out": BASE + 131072}) == SA_OK
    assert check(2, rows=1, **{"in": BASE, "out": BASE - 168}) == SA_OK
    assert check(2, rows=1, **{"in": BASE, "out": BASE - 160}) == SA_EINVAL
    # the alias bins of the header's two examples
    rng = np.random.default_rng(2404)
    for k1, want in ((6001, [6001, 4382, 1619, 7620, 2763]), (4096, [4096, 8192, 4096, 0, 4096])):
        rec = harm(plant(rng, k1, 1), **{k: v for k, v in GOOD.items()})
        assert rec["bin"][0].tolist() == want + [-1] * 5
        assert k1 != 4096 or (rec["power"][0, 2:5] == 0).all()


def test_touching_and_overlapping_ranges(check):
    """The records right behind the input and right in front of it are fine; moved into it by 8 and by 16 bytes they are
    refused; at addresses past 2^32 and near 2^47."""
    for X in (BASE + (1 << 30), (1 << 32) - 65536, 1 << 33):
        for field, rows in itertools.product((0, 1, 2), (1, 5, 4096)):
            n = sizes(field, rows)
            at = lambda pa, pb: check(field, rows=rows, **{"in": pa, "out": pb})      # noqa: E731
            assert at(X, X + n["in"]) == SA_OK and at(X, X - n["out"]) == SA_OK, (field, rows)
            assert at(X, X + n["in"] + 16) == SA_OK and at(X, X - n["out"] - 16) == SA_OK
            for by in (8, 16):
                assert at(X, X + n["in"] - by) == SA_EINVAL and at(X, X - n["out"] + by) == SA_EINVAL, (field, rows, by)
            assert at(X, X) == SA_EINVAL and at(X, X + 65536 - 8) == SA_EINVAL
            for off in (1, 2, 4, 8, 12, 16, 32):
                assert at(X + off, X + (1 << 40)) == (SA_OK if off % 16 == 0 else SA_EINVAL), off
                assert at(X, X + (1 << 40) + off) == (SA_OK if off % 8 == 0 else SA_EINVAL), off
            assert at(0, X) == SA_EINVAL and at(X, 0) == SA_EINVAL


def test_refusals_in_their_order(check, harm_lib):
    """1 negative rows, 2 the field, the NULL cfg and the parameters (also at rows 0), 3 the empty call, 4 the pointers: each
    refusal is shown to win over every later one by making the later ones wrong too."""
    bad = [dict(field=-1), dict(field=3), dict(cfg=False), dict(dc=-1), dict(dc=8193), dict(top=8194), dict(dc=100, top=100),
           dict(lo=3), dict(hi=8194), dict(lo=500, hi=500), dict(lo=501, hi=500), dict(fund=3), dict(fund=8193), dict(fund=-2),
           dict(span=-1), dict(span=65), dict(order=0), dict(order=11), dict(order=-2 ** 31), dict(span=2 ** 31 - 1),
           dict(dc=-2 ** 31, top=2 ** 31 - 1), dict(top=4000)]                       # hi 8193 is above a top of 4000
    wrong_ptrs = [dict(), {"in": 0, "out": 0}, {"in": BASE + 1, "out": BASE + 3}, {"in": BASE, "out": BASE}]
    for kw in [dict()] + bad:
        for p in wrong_ptrs:
            assert check(rows=-1, **dict(p, **kw)) == SA_ESHAPE, (kw, p)
            assert check(rows=-(1 << 31), **dict(p, **kw)) == SA_ESHAPE, (kw, p)
    for rows in (0, 1, 5, (1 << 31) - 1):
        for kw in bad:
            for p in wrong_ptrs:
                assert check(rows=rows, **dict(p, **kw)) == SA_EINVAL, (rows, kw, p)
    for p in wrong_ptrs:
        for field in (0, 1, 2):
            assert check(field=field, rows=0, **p) == SA_OK, p
    for p in wrong_ptrs[1:]:
        assert check(rows=1, **p) == SA_EINVAL, p
    assert check(rows=1) == SA_OK
    for kw in (dict(dc=0, top=1, lo=0, hi=1, span=0, order=1), dict(dc=0, top=1, lo=0, hi=1, fund=0, span=64, order=10), dict(field=2),
               dict(fund=4), dict(fund=8192), dict(top=4000, hi=4000), dict(lo=8192), dict(hi=5),
               dict(rows=(1 << 31) - 1, **{"in": 1 << 20, "out": 1 << 62})):
        assert check(**kw) == SA_OK, kw
    assert harm_lib.sa_harm_last_error() == b""                  # the check alone leaves the thread's text alone


def test_standalone_program_under_host_sanitizers(tmp_path):
    """tests/cpp/test_sa_harm_check.cpp + csrc/sa_harm_check.cpp, host only, under the address and undefined-behaviour
    sanitizers when they link here (a plain build otherwise: the program's own checks still run): every refusal in its order
    with the later ones wrong too, the known answers in bytes, touching and overlapping buffers at rows up to 2^31 - 1 and
    addresses past 2^32, near 2^47 and near 2^64.  Nothing is loaded into this process."""
    assert standalone_checks(tmp_path, "test_sa_harm_check", ["sa_harm_check.cpp"]) > 30000


# ----------------------------------------------------------------------------------------------------------- the wrappers
def test_the_wrappers_surface():
    """The Python entry points exist with the signatures of the issue; a bad parameter or field is SA_EINVAL before anything
    of the object or of a library is touched (the object here has neither)."""
    import inspect

    from fpga_real_time_fft_analyzer_amd import chain, frames
    cls = chain.SpectrumChain
    assert list(inspect.signature(frames.harm_of_rows).parameters) == ["points", "order", "span", "lo", "hi", "fund", "dc", "top", "field"]
    assert list(inspect.signature(cls.harmonics).parameters) == ["self", "t", "order", "span", "lo", "hi", "fund", "dc", "top", "field",
                                                                 "out"]
    assert list(inspect.signature(cls.harmonics_f32).parameters) == ["self", "x", "order", "span", "lo", "hi", "fund", "dc", "top", "group",
                                                                     "scale", "work", "out"]
    for fn in (frames.harm_of_rows, cls.harmonics, cls.harmonics_f32):
        sig = inspect.signature(fn).parameters
        assert (sig["order"].default, sig["span"].default, sig["top"].default) == (5, 3, 8193)
        assert all(sig[n].default is None for n in ("lo", "hi", "fund", "dc"))
    assert inspect.signature(cls.harmonics_f32).parameters["scale"].default == 1.0 / 2048.0
    assert list(inspect.signature(frames.harm_metrics).parameters) == ["records", "unit"]
    bare = object.__new__(cls)
    bad = [dict(order=0), dict(order=11), dict(order=2.0), dict(span=65), dict(span=True), dict(top=8194), dict(dc=-1), dict(lo=3),
           dict(hi=8194), dict(fund=3), dict(fund=-2), dict(lo="4"), dict(field="mag"), dict(field=0), dict(field=["peak"])]
    for kw in bad:
        with pytest.raises(chain.SpecanError) as e:
            bare.harmonics(None, **kw)
        assert e.value.code == SA_EINVAL and "tensor" not in str(e.value), (kw, str(e.value))
        if "field" not in kw:
            with pytest.raises(chain.SpecanError) as e:
                bare.harmonics_f32(None, **kw)
            assert e.value.code == SA_EINVAL and "tensor" not in str(e.value), (kw, str(e.value))
    for group in (0, 1, 3, 256, 2.0, True, "4"):
        with pytest.raises(chain.SpecanError) as e:
            bare.harmonics_f32(None, group=group)
        assert e.value.code == SA_EINVAL and "tensor" not in str(e.value), (group, str(e.value))
    with pytest.raises(chain.SpecanError) as e:                   # with good arguments the input's check does speak
        bare.harmonics_f32(None, 5, 3, group=4)
    assert e.value.code == SA_EINVAL and "tensor" in str(e.value)
    code, cfg = cls._harm_args(np.int64(10), 64, None, None, 100, 0, 4000, "power")
    assert code == 2 and [getattr(cfg, n) for n in GOOD] == [0, 4000, 0, 4000, 100, 64, 10]
    assert set(chain.reductions.FIELDS) == {None, "peak", "power"} and chain._HARM_WORDS == 42
