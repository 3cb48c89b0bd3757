"""CPU: the level histogram (include/specan_hist.h: sa_hist_f32 of libspecan_hist.so; SpectrumChain.level_hist and
persistence_f32) as far as no GPU is needed: the numpy mirror frames.hist_of_rows against probes whose expected counts are
worked out by hand below, never from the code under test; frames.level_edges_db by hand; the header against the built library
and the binding table abi.HIST_SIGNATURES; the kernels the five libraries hold; the refusals through sa_hist_check with
made-up addresses (every expected answer follows from the words of the header); the same arithmetic in a stand-alone program
under the host sanitizers.  What it links and its resource remarks: tests/test_reduction_libraries_cpu.py."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from conftest import N
from kernel_inventory import TABLE, inventory
from native import INCLUDE, compiles_as_c, declared, exported, standalone_checks
from reduction_libraries import BASE, SA_EINVAL, SA_ESHAPE, SA_OK, built, planted

FAR = BASE + (1 << 40)
HEADER = os.path.join(INCLUDE, "specan_hist.h")
NAMES = ["sa_hist_check", "sa_hist_f32", "sa_hist_last_error", "sa_hist_version"]
KERNELS = {f"hist_f32_kernel<{s}>" for s in range(1, 7)} | {"hist_zero_kernel"}
ONE_DOWN, ONE, ONE_UP = 0x3F7FFFFF, 0x3F800000, 0x3F800001    # 1.0f and its two neighbours


def hist(points, edges, **kw):
    from fpga_real_time_fft_analyzer_amd import frames
    got = frames.hist_of_rows(points, edges, **kw)
    assert got.dtype == np.uint32 and got.ndim == 3 and got.flags["C_CONTIGUOUS"] and got.shape[2] == len(edges) + 1
    return got


# ------------------------------------------------------------------------------------------------------------- the mirror
def test_planted_values_in_a_zero_row():
    """Edges (1, 10, 100): 0 -> level 0, 5 -> 1, 50 -> 2, 500 -> 3; every other bin is a zero in level 0."""
    pts = planted([(0, 5.0), (7, 50.0), (8, 500.0), (N - 1, 5.0)])
    got = hist(pts, [1.0, 10.0, 100.0])
    assert got.shape == (1, N, 4)
    for b, level in ((0, 1), (7, 2), (8, 3), (N - 1, 1), (1, 0), (9000, 0)):
        assert got[0, b].tolist() == [int(l == level) for l in range(4)], b
    assert got[0].sum(axis=0).tolist() == [N - 4, 2, 1, 1]
    got = hist(pts, [1.0, 10.0, 100.0], bucket=8)                 # columns of 8 bins: bins 0..7 hold the 5 and the 50, 8..15 the 500
    assert got.shape == (1, N // 8, 4)
    assert got[0, 0].tolist() == [6, 1, 1, 0] and got[0, 1].tolist() == [7, 0, 0, 1] and got[0, N // 8 - 1].tolist() == [7, 1, 0, 0]
    assert got[0, 2].tolist() == [8, 0, 0, 0]


def test_a_value_on_an_edge_is_in_the_level_above():
    pts = np.zeros((1, N), np.float32)
    pts.view(np.uint32)[0, [3, 700, 16383]] = (ONE, ONE_DOWN, ONE_UP)
    assert pts[0, 3] == 1.0 and pts[0, 700] < 1.0 < pts[0, 16383]
    got = hist(pts, [1.0])
    assert got[0, 3].tolist() == [0, 1] and got[0, 700].tolist() == [1, 0] and got[0, 16383].tolist() == [0, 1]
    assert got[0].sum(axis=0).tolist() == [N - 2, 2]


def test_specials_probe():
    """Edges (+0.0, 2.5, 1e30): NaN and +inf -> level 3 (the top edge is finite); -3.0 counts as 3.0 -> 2; 2.0 -> 1; the
    denormal 2^-149 is above the edge +0.0 -> 1; -0.0 is +0.0, equal to that edge -> 1, with every other zero: level 0 is
    empty."""
    pts = planted(((11, np.nan), (222, np.inf), (3333, -3.0), (4444, 2.0), (5555, 1e-45), (6666, -0.0)))
    assert pts.view(np.uint32)[0, 5555] == 1 and pts.view(np.uint32)[0, 6666] == 0x80000000
    got = hist(pts, [0.0, 2.5, 1e30])
    for b, level in ((11, 3), (222, 3), (3333, 2), (4444, 1), (5555, 1), (6666, 1), (0, 1)):
        assert got[0, b].tolist() == [int(l == level) for l in range(4)], b
    assert got[0].sum(axis=0).tolist() == [0, N - 3, 1, 2]
    # the denormal and +inf as edges: each value on its edge goes up; a negative NaN is a NaN
    pts.view(np.uint32)[0, 77] = 0xFFC00123
    got = hist(pts, [1e-45, np.inf])
    assert got[0, 5555].tolist() == [0, 1, 0] and got[0, 222].tolist() == [0, 0, 1] and got[0, 11].tolist() == [0, 0, 1]
    assert got[0, 77].tolist() == [0, 0, 1] and got[0, 6666].tolist() == [1, 0, 0]
    assert got[0].sum(axis=0).tolist() == [N - 6, 3, 3]


def test_equal_edges_give_empty_levels_and_two_levels():
    pts = np.zeros((2, N), np.float32)
    pts[0, :] = 1.0
    pts[1, :] = 1.5
    pts[1, 9] = 0.5
    got = hist(pts, [1.0, 1.0, 1.0, 2.0], group=2, bucket=2)
    assert got.shape == (1, N // 2, 5)
    assert got[0, 0].tolist() == [0, 0, 0, 4, 0] and got[0, 4].tolist() == [1, 0, 0, 3, 0]
    assert got[0].sum(axis=0).tolist() == [1, 0, 0, 2 * N - 1, 0]
    got = hist(pts, [1.25], group=1, bucket=64)                   # L = 2
    assert got.shape == (2, 256, 2)
    assert (got[0] == [64, 0]).all() and got[1, 0].tolist() == [1, 63] and (got[1, 1:] == [0, 64]).all()


def test_64_levels_one_value_per_level():
    """63 distinct edges 1..63; the value l + 0.5 planted at bin 100 l + 7 of a row of 0.25: one count in level l."""
    pts = np.full((1, N), 0.25, np.float32)
    pts[0, 100 * np.arange(64) + 7] = np.arange(64) + 0.5
    got = hist(pts, np.arange(1, 64, dtype=np.float32))
    for l in range(64):
        assert got[0, 100 * l + 7].tolist() == [int(k == l) for k in range(64)], l
    assert got[0].sum(axis=0).tolist() == [N - 63] + [1] * 63


def test_bins_outside_the_range_do_not_exist():
    rng = np.random.default_rng(1900)
    pts = np.exp(rng.uniform(-20.0, 20.0, size=(4, N))).astype(np.float32)
    edges = [1e-3, 1.0, 1e3]
    lo, hi = 1000, 3000
    before = hist(pts, edges, group=2, bucket=8, lo=lo, hi=hi)
    assert before.shape == (2, 250, 4)
    for v in (3e38, np.inf, np.nan, 0.0):
        loud = pts.copy()
        loud[:, lo - 1] = loud[:, hi] = v
        assert np.array_equal(hist(loud, edges, group=2, bucket=8, lo=lo, hi=hi), before), v
    loud = pts.copy()
    loud[:, lo] = 3e38                                            # inside: column 0 of both groups gains two in level 3
    after = hist(loud, edges, group=2, bucket=8, lo=lo, hi=hi)
    assert (after[:, 0, 3] >= 2).all() and np.array_equal(after[:, 1:], before[:, 1:])
    # the same cells as the full range's
    whole = hist(pts, edges, group=2, bucket=8)
    assert np.array_equal(whole[:, lo // 8:hi // 8], before)


def test_permutations_sums_and_additivity():
    rng = np.random.default_rng(1901)
    pts = np.exp(rng.uniform(-20.0, 20.0, size=(12, N))).astype(np.float32)
    pts[5] = rng.integers(0, 4, N)                                # massive ties, on the edges
    pts[7, ::5] *= -1.0
    edges = [0.0, 1.0, 1.0, 2.0, 3.0, 1e4]
    A, W = 6, 16
    want = hist(pts, edges, group=A, bucket=W)
    assert want.shape == (2, N // W, 7)
    assert (want.sum(axis=2, dtype=np.int64) == A * W).all()      # every (g, c) sums to A W
    assert not want[:, :, 0].any()                                # nothing is below +0.0
    for seed in (1, 2):
        p = np.random.default_rng(seed)
        rows = np.concatenate([p.permutation(A), A + p.permutation(A)])        # the rows of each group among themselves
        assert np.array_equal(hist(pts[rows], edges, group=A, bucket=W), want)
        inside = (np.arange(N).reshape(-1, W)[:, p.permutation(W)]).ravel()    # the bins inside every column
        assert np.array_equal(hist(pts[:, inside], edges, group=A, bucket=W), want)
    # the histogram of A = 6 is the sum of two histograms of A = 3 on the halves: what host-side persistence relies on
    halves = hist(pts, edges, group=3, bucket=W)
    assert np.array_equal(halves[0::2] + halves[1::2], want)
    # and of bucket 16 the sum of two columns of bucket 8
    narrow = hist(pts, edges, group=A, bucket=8)
    assert np.array_equal(narrow[:, 0::2] + narrow[:, 1::2], want)


def test_mirror_arguments():
    from fpga_real_time_fft_analyzer_amd import frames
    pts = np.zeros((4, N), np.float32)
    assert frames.hist_of_rows(np.zeros((0, N), np.float32), [1.0], bucket=64).shape == (0, 256, 2)
    assert frames.hist_of_rows(pts, (np.float32(1), 2, np.float64(3)), np.int64(2), np.int32(4), np.int16(4), np.int64(N)).shape == (2, 4095, 4)
    nan = float("nan")
    bad = [dict(edges=[]), dict(edges=list(range(64))), dict(edges=[nan]), dict(edges=[-1.0]), dict(edges=[-0.0]), dict(edges=[2.0, 1.0]),
           dict(edges=[True]), dict(edges=["1"]), dict(edges=1.0), dict(edges="12"), dict(edges=None), dict(group=0), dict(group=3),
           dict(group=(1 << 24) + 1), dict(group=2.0), dict(group=True), dict(bucket=0), dict(bucket=3), dict(bucket=128), dict(bucket=2.0),
           dict(lo=-1), dict(lo=5, hi=5), dict(hi=N + 1), dict(lo=1.0), dict(hi=True), dict(bucket=4, lo=2), dict(bucket=4, hi=N - 2)]
    for kw in bad:
        with pytest.raises(ValueError):
            frames.hist_of_rows(pts, **dict(dict(edges=[1.0]), **kw))
    for wrong in (pts.astype(np.float64), pts[:, :N // 2], pts[0], np.zeros((2, N, 2), np.float32)):
        with pytest.raises(ValueError):
            frames.hist_of_rows(wrong, [1.0])
    assert frames.hist_of_rows(pts, list(range(63))).shape == (1 * 4, N, 64)
    assert frames.hist_of_rows(pts, [1.0, np.inf, np.inf], group=4).shape == (1, N, 4)


def test_level_edges_db_by_hand():
    """top 1.0, span 40 dB, 4 levels: three edges 40, 20 and 0 dB below 1.0: 0.01, 0.1, 1.0, each rounded once."""
    from fpga_real_time_fft_analyzer_amd import frames
    e = frames.level_edges_db(1.0, 40.0, 4)
    assert e.dtype == np.float32 and e.shape == (3,)
    assert e[0] == np.float32(0.01) and e[1] == np.float32(0.1) and e[2] == np.float32(1.0)
    for top, span, levels in ((2000.0, 80.0, 64), (0.37, 100.0, 33), (1e-3, 6.0, 3), (7.0, 0.0, 5)):
        e = frames.level_edges_db(top, span, levels)
        assert e.shape == (levels - 1,) and e[-1] == np.float32(top), (top, span, levels)
        assert e[0] == np.float32(top * 10.0 ** (-span / 20.0))
        assert (np.diff(e.view(np.uint32).astype(np.int64)) >= 0).all()
        frames.hist_of_rows(np.zeros((1, N), np.float32), e)      # the histogram takes them
    one = frames.level_edges_db(3.5, 60.0, 2)
    assert one.shape == (1,) and one[0] == np.float32(3.5)
    for top, span, levels in ((0.0, 10, 4), (-1.0, 10, 4), (float("inf"), 10, 4), (1.0, -1, 4), (1.0, float("nan"), 4), (1.0, 10, 1),
                              (1.0, 10, 65), (1.0, 10, 4.0), (1.0, 10, True), ("1", 10, 4), (True, 10, 4)):
        with pytest.raises(ValueError):
            frames.level_edges_db(top, span, levels)


# ------------------------------------------------------------------------------------------------------------ the surface
@pytest.fixture(scope="module")
def hist_lib():
    return built("hist")


def _edges(values):
    return None if values is None else (ctypes.c_float * len(values))(*values)


@pytest.fixture(scope="module")
def check(hist_lib):
    def call(a_in=BASE, a_out=FAR, rows=4, group=2, log2w=0, nlev=None, edges=(1.0,), lo=0, hi=N):
        return hist_lib.sa_hist_check(a_in, a_out, rows, group, log2w, (len(edges) + 1 if edges is not None else 2) if nlev is None else nlev,
                                      _edges(edges), lo, hi)
    return call


def test_header_library_and_binding_table(hist_lib):
    """Name for name: declared in specan_hist.h = exported by libspecan_hist.so = bound in abi.HIST_SIGNATURES; nothing is in
    the five other tables or headers, which are what they were."""
    from fpga_real_time_fft_analyzer_amd import abi
    assert declared(HEADER) == NAMES
    assert [n for n in exported(abi.HIST_LIB_PATH) if "sa_" in n] == NAMES
    assert sorted(abi.HIST_SIGNATURES) == NAMES
    others = (abi.SIGNATURES, abi.EXT_SIGNATURES, abi.FOLD_SIGNATURES, abi.PEAKS_SIGNATURES, abi.RANK_SIGNATURES)
    assert not set(NAMES) & set().union(*others)
    assert [len(t) for t in others] == [45, 5, 4, 4, 4]
    for other in ("specan.h", "specan_ext.h", "specan_fold.h", "specan_peaks.h", "specan_rank.h"):
        assert not set(NAMES) & set(declared(os.path.join(INCLUDE, other))), other
    for name in NAMES:
        fn, (restype, argtypes) = getattr(hist_lib, name), abi.HIST_SIGNATURES[name]
        assert fn.argtypes is not None and list(fn.argtypes) == list(argtypes), name
        assert fn.restype is restype is (ctypes.c_char_p if name == "sa_hist_last_error" else ctypes.c_int), name
    assert hist_lib.sa_hist_version() == abi.SA_HIST_VERSION == 1 and abi.SA_HIST_LEVELS_MAX == 64
    text = open(HEADER).read()
    assert "#define SA_HIST_VERSION 1" in text and "#define SA_HIST_LEVELS_MAX 64" in text
    assert '#include "specan.h"' in text and len(re.findall(r"#\s*include", text)) == 1
    assert hist_lib.sa_hist_last_error() == b""
    assert os.path.basename(abi.HIST_LIB_PATH) == "libspecan_hist.so"
    assert os.path.dirname(abi.HIST_LIB_PATH) == os.path.dirname(abi.LIB_PATH)


def test_header_compiles_as_c99_pedantic(tmp_path):
    compiles_as_c(tmp_path, '#include "specan_hist.h"\n'
                   "int use(const float *p, uint32_t *o, const float *e) { return sa_hist_f32(p, o, 8, 4, 4, 32, e, 0, SA_N, 0)"
                   " + sa_hist_check(16, 32, 0, 1, 0, 2, e, 0, 1) + sa_hist_version() - SA_HIST_VERSION"
                   " + (sa_hist_last_error()[0] != 0) + SA_HIST_LEVELS_MAX - 64 + (o[0] > 0u); }\n")


def test_kernel_inventories(hist_lib):
    """libspecan_hist.so holds the six instantiations of the count, one per depth of the edge tree, and the kernel that zeroes
    the output of the sliced form, and nothing else; the other four libraries hold what they held."""
    from fpga_real_time_fft_analyzer_amd import abi
    assert inventory(abi.HIST_LIB_PATH) == KERNELS
    for path in (abi.LIB_PATH, abi.FOLD_LIB_PATH, abi.PEAKS_LIB_PATH, abi.RANK_LIB_PATH):
        if not os.path.exists(path):
            abi.build()
    assert inventory(abi.LIB_PATH) == set(TABLE)
    assert inventory(abi.FOLD_LIB_PATH) == {f"fold_mag_f32_kernel<{k}>" for k in range(7)}
    assert inventory(abi.PEAKS_LIB_PATH) == {f"peaks_f32_kernel<{f}>" for f in range(3)}
    assert inventory(abi.RANK_LIB_PATH) == {f"rank_f32_kernel<{f}>" for f in range(3)}
    design = open(os.path.join(os.path.dirname(INCLUDE), "DESIGN.md")).read()
    assert "hist_f32_kernel<STEPS>" in design and "hist_zero_kernel" in design


# -------------------------------------------------------------------------------------------------------------- the check
def out_bytes(rows, group, log2w, nlev, lo=0, hi=N):
    return (rows // group) * ((hi - lo) >> log2w) * nlev * 4


def test_known_answers_of_the_header(check):
    for rows, group, log2w, nlev, lo, hi, n_in, n_out in ((8, 4, 4, 32, 0, N, 524288, 262144), (3, 1, 0, 2, 16, 48, 196608, 768)):
        tag, kw = (rows, group, log2w, nlev), dict(rows=rows, group=group, log2w=log2w, edges=(1.0,) * (nlev - 1), lo=lo, hi=hi)
        assert (rows * 65536, out_bytes(rows, group, log2w, nlev, lo, hi)) == (n_in, n_out), tag
        assert check(BASE, BASE + n_in, **kw) == SA_OK, tag                    # out right behind in
        assert check(BASE, BASE - n_out, **kw) == SA_OK, tag                   # out right in front of in
        assert check(BASE, BASE + n_in - 4, **kw) == SA_EINVAL, tag            # out reaches into in
        assert check(BASE, BASE - n_out + 4, **kw) == SA_EINVAL, tag           # in reaches into out
        assert check(BASE, BASE, **kw) == SA_EINVAL, tag


def test_touching_and_overlapping_ranges(check):
    """out right behind in and right in front of it: touching is fine; moved into it by 1 byte (which also breaks the
    alignment), by 4 (the smallest overlap an aligned out can have) and by 16 it is refused.  The output may be the larger
    of the two (W = 1, L = 64: 64 counters per point)."""
    X = BASE + (1 << 34)
    for (rows, group), log2w, nlev in itertools.product(((1, 1), (4, 2), (6, 6), (5, 1)), (0, 3, 6), (2, 7, 64)):
        n_in, n_out = rows * 65536, out_bytes(rows, group, log2w, nlev)
        kw, tag = dict(rows=rows, group=group, log2w=log2w, edges=(2.0,) * (nlev - 1)), (rows, group, log2w, nlev)
        assert check(X, X + n_in, **kw) == SA_OK, tag
        assert check(X, X - n_out, **kw) == SA_OK, tag
        for by in (1, 4, 16):
            assert check(X, X + n_in - by, **kw) == SA_EINVAL, tag + (by,)
            assert check(X, X - n_out + by, **kw) == SA_EINVAL, tag + (by,)
        assert check(X, X - n_out - 16, **kw) == SA_OK, tag
        assert check(X, X + n_in + 16, **kw) == SA_OK, tag
        assert check(X, X + n_in // 2, **kw) == SA_EINVAL, tag                 # out begins inside in
        assert check(X, X - n_out // 2, **kw) == SA_EINVAL, tag                # in begins inside out
        for off in (1, 2, 4, 8, 12, 16, 32):
            assert check(BASE + off, FAR, **kw) == (SA_OK if off % 16 == 0 else SA_EINVAL), off
            assert check(BASE, FAR + off, **kw) == (SA_OK if off % 4 == 0 else SA_EINVAL), off
        for null in ("a_in", "a_out"):
            assert check(**kw, **{null: 0}) == SA_EINVAL, null


def test_refusals_in_their_order(check, hist_lib):
    """1 negative rows, 2 the scalar arguments and the edges (also at rows 0), 3 rows no multiple of the group, 4 the empty
    call, 5 the pointers: each refusal is shown to win over every later one by making the later ones wrong too."""
    nan, inf = float("nan"), float("inf")
    bad = [dict(group=0), dict(group=-1), dict(group=(1 << 24) + 1), dict(log2w=-1), dict(log2w=7), dict(nlev=1), dict(nlev=0),
           dict(nlev=65), dict(nlev=-3), dict(lo=-1), dict(lo=5, hi=5), dict(lo=6, hi=5), dict(hi=N + 1), dict(lo=N, hi=N + 1),
           dict(log2w=2, lo=2), dict(log2w=2, hi=N - 2), dict(log2w=6, lo=32, hi=96), dict(edges=None), dict(edges=(nan,)),
           dict(edges=(-1.0,)), dict(edges=(-0.0,)), dict(edges=(1.0, 2.0, nan)), dict(edges=(2.0, 1.0)), dict(edges=(0.0, inf, 3e38)),
           dict(edges=(1.0,) * 62 + (0.5,)), dict(edges=(-inf,))]
    wrong_ptrs = [dict(), dict(a_in=0, a_out=0), dict(a_in=BASE + 1, a_out=BASE + 3), dict(a_in=BASE, a_out=BASE)]
    # 1: before bad arguments, a group that does not divide, and bad pointers
    for kw in [dict(), dict(group=3)] + bad:
        for p in wrong_ptrs:
            assert check(**dict(dict(kw, **p), rows=-1)) == SA_ESHAPE, (kw, p)
            assert check(**dict(dict(kw, **p), rows=-(1 << 31))) == SA_ESHAPE, (kw, p)
    # 2: before the group that does not divide, the empty call and the pointers
    for rows in (0, 1, 4, 5, (1 << 31) - 1):
        for kw in bad:
            for p in wrong_ptrs:
                assert check(**dict(dict(dict(group=2), **kw, **p), rows=rows)) == SA_EINVAL, (rows, kw, p)
    # 3: rows no multiple of the group, before the pointers
    for rows, group in ((5, 2), (1, 2), (4, 3), ((1 << 31) - 1, 2), (1 << 24, (1 << 24) - 1)):
        for p in wrong_ptrs:
            assert check(rows=rows, group=group, **p) == SA_ESHAPE, (rows, group, p)
    # 4: the empty call is SA_OK whatever the pointers are (0 is a multiple of every group)
    for p in wrong_ptrs:
        for group in (1, 2, 1 << 24):
            assert check(rows=0, group=group, **p) == SA_OK, p
    # 5: the pointers, last
    for p in wrong_ptrs[1:]:
        assert check(**p) == SA_EINVAL, p
    assert check() == SA_OK
    # within 2: nlev is judged before the edges are read -- a null array with a bad nlev is the bad nlev's refusal, and the call
    # returns at all with nlev = 65 and an array of one entry (the stand-alone program holds every array at exactly L - 1
    # entries under the address sanitizer)
    assert check(nlev=65, edges=(1.0,)) == SA_EINVAL and check(nlev=1, edges=None) == SA_EINVAL
    # the edges of every scalar that are good
    for kw in (dict(group=1), dict(rows=1 << 24, group=1 << 24, a_in=1 << 20, a_out=1 << 62), dict(log2w=6, lo=64, hi=128),
               dict(lo=N - 1, hi=N), dict(lo=0, hi=1), dict(edges=(0.0,)), dict(edges=(inf,)), dict(edges=(0.0, 0.0, inf, inf)),
               dict(edges=tuple(float(v) for v in range(63))), dict(edges=(1e-45, 1e-45)), dict(rows=(1 << 31) - 1, group=1, a_in=1 << 20, a_out=1 << 62)):
        assert check(**kw) == SA_OK, kw
    assert hist_lib.sa_hist_last_error() == b""                   # the check alone leaves the thread's text alone


def test_standalone_program_under_host_sanitizers(tmp_path):
    """tests/cpp/test_sa_hist_check.cpp + csrc/sa_hist_check.cpp, host only, under the address and undefined-behaviour
    sanitizers when they link here (a plain build otherwise: the program's own checks still run): the same arithmetic at rows
    up to 2^31 - 1, groups up to 2^24 and addresses near 2^47 and 2^64, every array of edges exactly L - 1 long.  Nothing is
    loaded into this process."""
    assert standalone_checks(tmp_path, "test_sa_hist_check", ["sa_hist_check.cpp"]) > 100000


# ----------------------------------------------------------------------------------------------------------- the wrappers
def test_the_wrappers_surface():
    """The Python entry points exist; a bad edge set, group, bucket or range is SA_EINVAL before anything of the object or of
    a library is touched (the object here has neither)."""
    import inspect
    from fpga_real_time_fft_analyzer_amd import chain
    cls = chain.SpectrumChain
    assert list(inspect.signature(cls.level_hist).parameters) == ["self", "t", "edges", "group", "bucket", "lo", "hi", "out"]
    assert list(inspect.signature(cls.persistence_f32).parameters) == ["self", "x", "edges", "group", "bucket", "lo", "hi", "scale", "work", "out"]
    assert inspect.signature(cls.level_hist).parameters["bucket"].default == 1
    assert inspect.signature(cls.persistence_f32).parameters["bucket"].default == 16
    assert inspect.signature(cls.persistence_f32).parameters["scale"].default == 1.0 / 2048.0
    bare = object.__new__(cls)
    nan = float("nan")
    bad = [dict(edges=[]), dict(edges=list(range(64))), dict(edges=[nan]), dict(edges=[-1.0]), dict(edges=[2.0, 1.0]), dict(edges=[True]),
           dict(edges=5.0), dict(edges=None), dict(edges="1"), dict(group=0), dict(group=(1 << 24) + 1), dict(group=2.0), dict(group=True),
           dict(group="4"), dict(bucket=0), dict(bucket=3), dict(bucket=128), dict(bucket=2.0), dict(bucket=True), dict(lo=-1),
           dict(lo=7, hi=7), dict(hi=N + 1), dict(lo=0.0), dict(hi=True), dict(bucket=4, lo=2), dict(bucket=16, hi=N - 8)]
    for method in (bare.level_hist, bare.persistence_f32):
        for kw in bad:
            with pytest.raises(chain.SpecanError) as e:
                method(None, **dict(dict(edges=[1.0]), **kw))
            assert e.value.code == SA_EINVAL and "tensor" not in str(e.value), (kw, str(e.value))
        with pytest.raises(chain.SpecanError) as e:               # with good arguments the input's check does speak
            method(None, [1.0, 2.0], group=4)
        assert e.value.code == SA_EINVAL and "tensor" in str(e.value)
    assert cls._hist_args([1, np.float32(2.5)], None, 16, 0, N) == (4, (1.0, 2.5))
    assert cls._hist_args(np.array([0.0, np.inf], np.float32), np.int64(3), 1, np.int32(5), 6) == (0, (0.0, float("inf")))
    assert cls._hist_args((0.1,), 1 << 24, 64, 64, 128) == (6, (float(np.float32(0.1)),))
