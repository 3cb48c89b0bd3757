"""CPU: the percentile traces (include/specan_hold.h: sa_hold_f32 of libspecan_hold.so; SpectrumChain.hold_ranks and hold_f32)
as far as no GPU is needed: the numpy mirror frames.holds_of_rows against probes whose expected bits are worked out by hand
below, never from the code under test; the header against the built library and the binding table abi.HOLD_SIGNATURES; what
the library links, the kernels it holds and their resource remarks; the Makefile lines that build it; the refusals through
sa_hold_check with made-up addresses (every expected answer follows from the words of the header); the same arithmetic in a
stand-alone program under the host sanitizers; and the shapes of the past-4-GiB cases of tests/test_gpu_hold_offsets.py."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import offset_cases
from conftest import N
from kernel_inventory import inventory, unit_text
from native import CSRC, INCLUDE, compiles_as_c, declared, exported, needed, standalone_checks, undefined
from reduction_libraries import BASE, LIBRARIES, QUIET, SA_EINVAL, SA_ESHAPE, SA_OK, bits, key, records_of
from test_reduction_libraries_cpu import figures

FAR = BASE + (1 << 40)
HEADER = os.path.join(INCLUDE, "specan_hold.h")
NAMES = ["sa_hold_check", "sa_hold_f32", "sa_hold_last_error", "sa_hold_version"]
UNITS = ("hold_f32.hip", "sa_hold_check.cpp")
ONE, ONE_UP = 0x3F800000, 0x3F800001                   # 1.0f and the next float above it
CLASSES = (8, 16, 32, 64, 128)                         # the register classes AMAX of csrc/sa_hold.hpp
ROW = 65536                                            # bytes of a row of magnitudes
# the specials of one bin over six frames and their keys ascending: -0.0 as zero, the denormal 2^-149 (bits 1), 2.0, |-3.0|,
# +inf, the NaN
SPECIALS = (np.nan, np.inf, -3.0, 2.0, 1e-45, -0.0)
SPECIALS_SORTED = [0x0, 0x1, 0x40000000, 0x40400000, 0x7F800000, 0x7FC00000]
# the past-4-GiB calls of tests/test_gpu_hold_offsets.py: (field, A, q)
OFFSET_CALLS = ((None, 2, 2), ("power", 2, 1))


def hold_class(group):
    """the smallest class that holds a group, as csrc/sa_hold.hpp has it"""
    return next(c for c in CLASSES if c >= group)


def hold_bins(amax, field):
    """adjacent bins of a thread, as csrc/sa_hold.hpp has it: one 16-byte load in the classes of 16 keys or fewer"""
    return (4 if field is None else 2) if amax <= 16 else 1


def offset_shape(field, A, q):
    """(period in rows, rows) of a past-4-GiB call by the rules of tests/offset_cases.py: the deciding tensor is the smaller
    of the input's A rows and the output's q rows per group, and the batch the smallest at which its last row (group) starts
    at or beyond 2^32, plus EXTRA."""
    per_group = {"in": A * ROW * (1 if field is None else 2), "out": q * ROW}
    return offset_cases.period(A), offset_cases.batch(per_group, A)


def traces(points, ranks, group, **kw):
    """the mirror's result as keys, uint32 [G, q, N]"""
    from fpga_real_time_fft_analyzer_amd import frames
    got = frames.holds_of_rows(points, ranks, group, **kw)
    assert got.dtype == np.float32 and got.shape == (points.shape[0] // group, len(ranks), N) and got.flags["C_CONTIGUOUS"]
    return bits(got)


# ------------------------------------------------------------------------------------------------------------- the mirror
def test_last_bit_probe():
    """A rows of 1.0, in one of them one bin one ulp up: that bin's maximum alone is the larger float."""
    up = np.nextafter(np.float32(1), np.float32(2), dtype=np.float32)
    assert key(up) == ONE_UP and key(1) == ONE
    for A, row, at in ((2, 0, 0), (3, 2, 7777), (5, 1, N - 1), (128, 77, 4096)):
        pts = np.ones((A, N), np.float32)
        pts[row, at] = up
        got = traces(pts, [A - 1, A - 2, 0], A)
        want = np.full((1, 3, N), ONE, np.uint32)
        want[0, 0, at] = ONE_UP
        assert np.array_equal(got, want), A


def test_specials_probe():
    """NaN above +inf above every finite value, -3.0 as 3.0, the denormal kept above zero, -0.0 as zero: one bin holds the six
    over six frames, in every order of the frames the sorted keys are the same; the answers lie on both sides of bit 30 and
    differ in bit 0 alone (0x0 and 0x1)."""
    for order in ((0, 1, 2, 3, 4, 5), (5, 4, 3, 2, 1, 0), (2, 5, 0, 3, 1, 4)):
        pts = np.zeros((6, N), np.float32)
        pts[:, 1234] = np.array(SPECIALS, np.float32)[list(order)]
        got = traces(pts, list(range(6)), 6)
        assert got[0, :, 1234].tolist() == SPECIALS_SORTED
        assert not got[0, :, :1234].any() and not got[0, :, 1235:].any()
    pts = np.zeros((2, N), np.float32)
    pts.view(np.uint32)[1, 77] = 0xFFC00123                       # a negative NaN: the sign cleared, the payload kept
    assert traces(pts, [1, 0], 2)[0, :, 77].tolist() == [0x7FC00123, 0]


def test_ties_that_straddle_a_rank():
    """Seven frames of a bin: 2, 5, 5, 5, 5, 9, 9 in any order -- ranks 1..4 are the 5 on both sides of the median, rank 0 the 2
    and ranks 5, 6 the 9; a neighbouring bin holds seven equal values."""
    pts = np.zeros((7, N), np.float32)
    pts[:, 100] = (5, 9, 5, 2, 5, 9, 5)
    pts[:, 101] = 4.0
    got = traces(pts, [0, 1, 3, 4, 5, 6], 7)
    assert got[0, :, 100].tolist() == [key(v) for v in (2, 5, 5, 5, 9, 9)]
    assert got[0, :, 101].tolist() == [key(4)] * 6


def test_repeated_and_unsorted_ranks():
    """Frame a holds a + bin / 16384 in every bin (exact in float32 below 256): the key at rank r of bin i is r + i / 16384."""
    A = 15
    pts = (np.arange(A, dtype=np.float32)[:, None] + np.arange(N, dtype=np.float32)[None, :] / N).astype(np.float32)
    ranks = [9, 3, 9, A - 1, 0, 3, 7, 9]
    want = bits((np.array(ranks, np.float32)[:, None] + np.arange(N, dtype=np.float32)[None, :] / N).astype(np.float32))
    assert np.array_equal(traces(pts, ranks, A)[0], want)
    assert np.array_equal(traces(pts[::-1], ranks, A)[0], want)   # the frames descending: the same sorted keys


def test_any_permutation_of_a_groups_rows_and_other_groups():
    """The rows of a group in any order give the same output; what the other groups hold changes nothing."""
    rng = np.random.default_rng(2700)
    A, G = 5, 3
    pts = np.exp(rng.uniform(-60.0, 60.0, size=(G * A, N))).astype(np.float32)
    pts[A:2 * A] = rng.integers(0, 3, (A, N))                     # massive ties in group 1
    pts[2 * A:, ::5] *= -1.0
    ranks = [0, 2, A - 1, 1]
    want = traces(pts, ranks, A)
    for seed in (1, 2):
        shuffled = pts.reshape(G, A, N).copy()
        for g in range(G):
            shuffled[g] = shuffled[g][np.random.default_rng(seed + g).permutation(A)]
        assert np.array_equal(traces(shuffled.reshape(G * A, N), ranks, A), want)
    for g in range(G):
        assert np.array_equal(traces(pts[g * A:(g + 1) * A], ranks, A)[0], want[g])
        for v in (np.nan, np.inf, 0.0):
            loud = np.full_like(pts, v)
            loud[g * A:(g + 1) * A] = pts[g * A:(g + 1) * A]
            assert np.array_equal(traces(loud, ranks, A)[g], want[g]), (g, v)
    # positive data: the keys are the bits, and a rank is np.sort along the frames
    assert np.array_equal(want[0], np.sort(bits(pts[:A]), axis=0)[ranks])


def test_records_and_arguments():
    from fpga_real_time_fft_analyzer_amd import frames
    rng = np.random.default_rng(2701)
    pts = np.exp(rng.uniform(-60.0, 60.0, size=(6, N))).astype(np.float32)
    ranks = [1, 0, 2]
    whole = traces(pts, ranks, 3)
    # records: the named float is the point, the other one (a NaN) is never looked at
    for field in ("peak", "power"):
        assert np.array_equal(traces(records_of(pts, field), ranks, 3, field=field), whole), field
    assert frames.holds_of_rows(np.zeros((0, N), np.float32), [0, 1], 2).shape == (0, 2, N)
    assert frames.HOLD_Q_MAX == 8 and frames.HOLD_GROUP_MAX == 128
    for rows in (5, 4, 1):
        with pytest.raises(ValueError, match=r"the rows \(%d\) must be a multiple of 3" % rows):
            frames.holds_of_rows(pts[:rows], ranks, 3)
    for wrong in (pts.astype(np.float64), pts[:, :N // 2], pts[0], np.zeros((2, N, 2), np.float32)):
        with pytest.raises(ValueError):
            frames.holds_of_rows(wrong, [0], 2)
    with pytest.raises(ValueError):
        frames.holds_of_rows(pts, [0], 2, field="peak")            # records are [R, 16384, 2]
    got = frames.holds_of_rows(pts, (np.int64(1), np.int16(0)), np.int32(3))
    assert np.array_equal(bits(got), bits(frames.holds_of_rows(pts, np.array([1, 0]), 3)))


BAD_ARGS = [(dict(group=1), "group must be 2..128"), (dict(group=0), "group must be 2..128"), (dict(group=129), "group must be 2..128"),
            (dict(group=-4), "group must be 2..128"), (dict(group=2.0), "group must be an int"), (dict(group=True), "group must be an int"),
            (dict(group="4"), "group must be an int"), (dict(group=None), "group must be an int"),
            (dict(ranks=[]), "ranks must be a sequence of 1..8 ints"), (dict(ranks=list(range(9)), group=16), "ranks must be a sequence"),
            (dict(ranks=3), "ranks must be a sequence"), (dict(ranks="12"), "ranks must be a sequence"),
            (dict(ranks=None), "ranks must be a sequence"),
            (dict(ranks=[4]), "a rank must be an int in 0..3"), (dict(ranks=[-1]), "a rank must be an int in 0..3"),
            (dict(ranks=[True]), "a rank must be an int in 0..3"), (dict(ranks=[1.0]), "a rank must be an int in 0..3"),
            (dict(ranks=[0, 127], group=127), "a rank must be an int in 0..126"),
            (dict(field="mag"), "field must be None, 'peak' or 'power'"), (dict(field=0), "field must be"),
            (dict(field=["peak"]), "field must be")]


def test_hold_args_refusals_by_text():
    """frames._hold_args: the group, then the ranks, the field last; one text per rule."""
    from fpga_real_time_fft_analyzer_amd import frames
    for kw, words in BAD_ARGS:
        with pytest.raises(ValueError) as e:
            frames._hold_args(**dict(dict(ranks=[0], group=4, field=None), **kw))
        assert words in str(e.value), (kw, str(e.value))
    # the order: a bad group before bad ranks before a bad field
    for kw, words in ((dict(group=1, ranks=[], field="x"), "group must be"), (dict(group=4, ranks=[9], field="x"), "a rank must be")):
        with pytest.raises(ValueError) as e:
            frames._hold_args(**kw)
        assert words in str(e.value)
    assert frames._hold_args([np.int64(1), 0], np.int32(2), None) == ((1, 0), 2)
    assert frames._hold_args((127,) * 8, 128, "power") == ((127,) * 8, 128)
    assert frames._hold_args(np.array([0, 2]), 3, "peak") == ((0, 2), 3)


def test_the_wrappers_surface():
    """The Python entry points exist; a bad rank set, quantile, group or field is SA_EINVAL with the words of the rule before
    anything of the object or of a library is touched (the object here has neither)."""
    from fpga_real_time_fft_analyzer_amd import chain, holds, reductions
    cls = chain.SpectrumChain
    assert cls.__bases__ == (reductions.Reductions, holds.Holds)
    assert callable(cls.hold_ranks) and callable(cls.hold_f32)
    bare = object.__new__(cls)
    for kw, words in BAD_ARGS:
        with pytest.raises(chain.SpecanError) as e:
            bare.hold_ranks(None, **dict(dict(ranks=[0], group=4), **kw))
        assert e.value.code == SA_EINVAL and words in str(e.value) and "tensor" not in str(e.value), (kw, str(e.value))
    for kw, words in [(kw, words) for kw, words in BAD_ARGS if "group" in kw and "ranks" not in kw] + [
            (dict(q=-0.1), "q must be a number in 0..1"), (dict(q=1.5), "q must be a number in 0..1"),
            (dict(q=float("nan")), "q must be a number in 0..1"), (dict(q="0.5"), "q must be a number in 0..1"),
            (dict(q=None), "q must be a number in 0..1"), (dict(q=True), "q must be a number in 0..1"),
            (dict(q=[]), "q must be a number or a sequence of 1..8 numbers"), (dict(q=[0.1] * 9), "q must be a number or a sequence"),
            (dict(q=[0.5, 2.0]), "q must be a number in 0..1")]:
        with pytest.raises(chain.SpecanError) as e:
            bare.hold_f32(None, **kw)
        assert e.value.code == SA_EINVAL and words in str(e.value) and "tensor" not in str(e.value), (kw, str(e.value))
    for call in (lambda: bare.hold_ranks(None, [0, 1], 2), lambda: bare.hold_f32(None, [0.0, 0.5], group=5)):
        with pytest.raises(chain.SpecanError) as e:               # with good arguments the input's check does speak
            call()
        assert e.value.code == SA_EINVAL and "tensor" in str(e.value)
    assert cls._hold_args([np.int64(1), 0], np.int32(2), None) == (0, (1, 0), 2)
    assert cls._hold_args((4,), 5, "peak") == (1, (4,), 5) and cls._hold_args(np.array([0]), 128, "power") == (2, (0,), 128)
    # floor(q (A - 1)): the lower median of 16 frames is rank 7, of 15 rank 7, of 5 rank 2; 0 and 1 are the two holds
    assert cls._hold_quantile_ranks(0.5, 16) == (7,) and cls._hold_quantile_ranks([0.0, 0.5, 1.0], 15) == (0, 7, 14)
    assert cls._hold_quantile_ranks((0.5, 0.9), 5) == (2, 3)


# ------------------------------------------------------------------------------------------------------------ the surface
@pytest.fixture(scope="module")
def hold_lib():
    from fpga_real_time_fft_analyzer_amd import abi
    if not os.path.exists(abi.HOLD_LIB_PATH):
        abi.build()
    return abi.hold_lib()


def _ranks(values):
    return None if values is None else (ctypes.c_int32 * len(values))(*values)


@pytest.fixture(scope="module")
def check(hold_lib):
    def call(field=0, a_in=BASE, a_out=FAR, rows=6, group=3, q=None, ranks=(0,)):
        return hold_lib.sa_hold_check(field, a_in, a_out, rows, group, (len(ranks) if ranks is not None else 1) if q is None else q,
                                      _ranks(ranks))
    return call


def test_header_library_and_binding_table(hold_lib):
    """Name for name: declared in specan_hold.h = exported by libspecan_hold.so = bound in abi.HOLD_SIGNATURES; nothing is in
    the other tables or headers, which are what they were; the library is no row of abi.LIBRARIES."""
    from fpga_real_time_fft_analyzer_amd import abi
    assert declared(HEADER) == NAMES
    assert [n for n in exported(abi.HOLD_LIB_PATH) if "sa_" in n] == NAMES
    assert sorted(abi.HOLD_SIGNATURES) == NAMES
    others = [abi.SIGNATURES, abi.EXT_SIGNATURES] + [table for _, table in abi.LIBRARIES.values()]
    assert not set(NAMES) & set().union(*others)
    assert [len(t) for t in others] == [45, 5] + [4] * 9
    assert "hold" not in abi.LIBRARIES and list(abi.LIBRARIES) == list(LIBRARIES)
    for other in os.listdir(INCLUDE):
        if other != "specan_hold.h":
            assert not set(NAMES) & set(declared(os.path.join(INCLUDE, other))), other
    for name in NAMES:
        fn, (restype, argtypes) = getattr(hold_lib, name), abi.HOLD_SIGNATURES[name]
        assert fn.argtypes is not None and list(fn.argtypes) == list(argtypes), name
        assert fn.restype is restype is (ctypes.c_char_p if name == "sa_hold_last_error" else ctypes.c_int), name
    assert hold_lib.sa_hold_version() == abi.SA_HOLD_VERSION == 1 and abi.SA_HOLD_Q_MAX == 8 and abi.SA_HOLD_GROUP_MAX == 128
    text = open(HEADER).read()
    assert "#define SA_HOLD_VERSION 1" in text and "#define SA_HOLD_Q_MAX 8" in text and "#define SA_HOLD_GROUP_MAX 128" in text
    assert '#include "specan.h"' in text and "#include \"specan_rank.h\"" not in text
    assert (abi.SA_HOLD_IN_MAG, abi.SA_HOLD_IN_POINT_PEAK, abi.SA_HOLD_IN_POINT_POWER) == (0, 1, 2) == \
        (abi.SA_RANK_IN_MAG, abi.SA_RANK_IN_POINT_PEAK, abi.SA_RANK_IN_POINT_POWER)
    assert hold_lib.sa_hold_last_error() == b""
    assert abi.HOLD_LIB_PATH == os.path.join(os.path.dirname(abi.LIB_PATH), "libspecan_hold.so")
    assert abi.hold_lib() is hold_lib and "libspecan_hold.so" in abi.hold_lib.__doc__ and "specan_hold.h" in abi.hold_lib.__doc__


def test_header_compiles_as_c99_pedantic(tmp_path):
    compiles_as_c(tmp_path, '#include "specan_hold.h"\n'
                  "int use(const void *p, float *o, const int32_t *r) { return sa_hold_f32(p, SA_HOLD_IN_POINT_POWER, o, 8, 4, 2, r,"
                  " 0) + sa_hold_check(SA_HOLD_IN_MAG, 16, 32, 0, 2, 1, r) + sa_hold_version() - SA_HOLD_VERSION"
                  " + (sa_hold_last_error()[0] != 0) + SA_HOLD_Q_MAX - 8 + SA_HOLD_GROUP_MAX - 128 + SA_HOLD_IN_POINT_PEAK - 1"
                  " + (o[0] > 0.0f); }\n")


def test_library_links_hip_alone_and_reads_no_environment(hold_lib):
    """What tests/test_reduction_libraries_cpu.py holds the nine libraries to, for this one: loaded with the HIP runtime and
    nothing of torch, the oracle or the other libraries; no environment; its units include their own two headers and
    specan.h alone; one launch; no atomics, no FP-mode change, nothing zeroed; both entry points through the one check."""
    from fpga_real_time_fft_analyzer_amd import abi
    libs = needed(abi.HOLD_LIB_PATH)
    for other in ("torch", "oracle", "specan_hip", *(f"specan_{y}" for y in LIBRARIES)):
        assert other not in libs, libs
    assert "amdhip64" in libs
    assert "getenv" not in undefined(abi.HOLD_LIB_PATH)
    text = unit_text(UNITS[0]) + unit_text(UNITS[1])
    assert all(name in text for name in NAMES) and "sa_hold_check_call" in text
    assert "getenv" not in text and "environ" not in text.replace("environment", "")
    assert not re.search(r'#\s*include\s+"(?!sa_hold\.hpp|\.\./\.\./include/specan_hold\.h|specan\.h)', text)
    code = re.sub(r"//.*", "", open(os.path.join(CSRC, UNITS[0])).read())
    for word in QUIET + ("__shared__", "__syncthreads"):
        assert word not in code, word
    assert len(re.findall(r"hipLaunchKernelGGL", code)) == 1 and "extern __shared__" not in code
    assert len(re.findall(r"sa_hold_check_call\(", unit_text(UNITS[1]))) >= 2
    assert len(re.findall(r"sa_hold_check_call\(", code)) == 1
    # the groups are on the grid's x: y holds 65535 at most, and a call may have 2^24 groups
    assert re.search(r"dim3 grid\(\(unsigned\)\(rows / group\),", code) and re.search(r"size_t g = blockIdx\.x;", code)


def test_kernel_inventory(hold_lib):
    """libspecan_hold.so holds one instantiation per input layout and register class, and nothing else."""
    from fpga_real_time_fft_analyzer_amd import abi
    assert inventory(abi.HOLD_LIB_PATH) == {f"hold_f32_kernel<{f}, {amax}>" for f in range(3) for amax in CLASSES}
    hpp = open(os.path.join(CSRC, "sa_hold.hpp")).read()
    assert "kHoldThreads = 256" in hpp and "kHoldClassMin = 8" in hpp and "kHoldWideMax = 16" in hpp
    assert [hold_class(a) for a in (2, 8, 9, 16, 17, 32, 33, 64, 65, 128)] == [8, 8, 16, 16, 32, 32, 64, 64, 128, 128]


# occupancy (waves per SIMD) of the instantiations of a class, magnitudes / records, and the most VGPRs of any kernel: the
# figures the compile prints
OCCUPANCY = {8: (8, 8), 16: (5, 8), 32: (8, 8), 64: (4, 4), 128: (2, 2)}
VGPRS_MAX = 219


def test_resource_remarks_and_makefile_lines():
    """The lines of the Makefile that build the library, by the regexes tests/test_reduction_libraries_cpu.py spells for the
    nine; then the compiler's figures for the fifteen kernels: no scratch, no SGPR or VGPR spill, no LDS at all, and the
    occupancy and VGPR maximum DESIGN.md section 4.25 records."""
    x, X = "hold", "HOLD"
    make = open(os.path.join(CSRC, "Makefile")).read()
    for pin in (r"^%s_SRCS = %s %s$" % (X, re.escape(UNITS[0]), re.escape(UNITS[1])), r"^%s_OBJS = " % X,
                r"^%s_OUT = \.\./libspecan_%s\.so$" % (X, x),
                r"^\$\(X_OUT\): \$\(X_OBJS\)\n\t\$\(HIPCC\) \$\(CXXFLAGS\) -shared \$\(X_OBJS\) -o \$@$".replace("X_", X + "_"),
                r"^all:.*\$\(%s_OUT\)" % X, r"^UNITS = .*\$\(%s_SRCS\)" % X, r"^clean:\n\trm .*\$\(%s_OUT\)" % X,
                r"^RESOURCE = .*resource-%s-f32" % x, r"^resource-%s-f32: UNITS = %s$" % (x, re.escape(UNITS[0]))):
        assert re.search(pin, make, re.M), pin
    assert f"libspecan_{x}.so" in "\n".join(make.split("\n", 2)[:2])
    got = figures(UNITS[0])
    assert len(got) == 15 and all("hold_f32_kernel" in name for name, _ in got), [name for name, _ in got]
    for what in ("ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]"):
        assert [f[what] for _, f in got] == [0] * 15, what
    vgprs = {name: f["VGPRs"] for name, f in got}
    print("FIGURE hold (DESIGN.md section 4.25) VGPRs", list(vgprs.values()), "occupancy", [f["Occupancy [waves/SIMD]"] for _, f in got])
    for name, f in got:
        field, amax = map(int, re.search(r"hold_f32_kernelILi(\d)ELi(\d+)E", name).groups())
        assert f["Occupancy [waves/SIMD]"] == OCCUPANCY[amax][1 if field else 0], (name, f)
    assert max(vgprs.values()) == VGPRS_MAX
    design = open(os.path.join(os.path.dirname(INCLUDE), "DESIGN.md")).read()
    assert "### 4.25" in design and str(VGPRS_MAX) in design.split("### 4.25", 1)[1]


# -------------------------------------------------------------------------------------------------------------- the check
def in_bytes(field, rows):
    return rows * ROW * (2 if field else 1)


def test_known_answers_of_the_header(check):
    for field, rows, group, q, n_in, n_out in ((0, 6, 3, 8, 393216, 1048576), (2, 2, 2, 1, 262144, 65536),
                                               (1, 256, 128, 2, 33554432, 262144)):
        tag, kw = (field, rows, group, q), dict(rows=rows, group=group, ranks=(0,) * q)
        assert (in_bytes(field, rows), rows // group * q * ROW) == (n_in, n_out), tag
        assert check(field, BASE, BASE + n_in, **kw) == SA_OK, tag                 # out right behind in
        assert check(field, BASE, BASE - n_out, **kw) == SA_OK, tag                # out right in front of in
        assert check(field, BASE, BASE + n_in - 16, **kw) == SA_EINVAL, tag        # out reaches into in
        assert check(field, BASE, BASE - n_out + 16, **kw) == SA_EINVAL, tag       # in reaches into out
        assert check(field, BASE, BASE, **kw) == SA_EINVAL, tag


def test_touching_and_overlapping_ranges(check):
    """out right behind in and right in front of it: touching is fine; moved into it by 1 and by 4 bytes (which also break the
    alignment) and by 16 (the smallest overlap an aligned out can have) it is refused."""
    X = BASE + (1 << 30)
    for field, (rows, group), q in itertools.product((0, 1, 2), ((2, 2), (9, 3), (256, 128), (10, 5)), (1, 3, 8)):
        n_in, n_out, kw = in_bytes(field, rows), rows // group * q * ROW, dict(rows=rows, group=group, ranks=(0,) * q)
        tag = (field, rows, group, q)
        assert check(field, X, X + n_in, **kw) == SA_OK, tag
        assert check(field, X, X - n_out, **kw) == SA_OK, tag
        for by in (1, 4, 16):
            assert check(field, X, X + n_in - by, **kw) == SA_EINVAL, tag + (by,)
            assert check(field, X, X - n_out + by, **kw) == SA_EINVAL, tag + (by,)
        assert check(field, X, X - n_out - 16, **kw) == SA_OK, tag
        assert check(field, X, X + n_in + 16, **kw) == SA_OK, tag
        assert check(field, X, X + n_in // 2, **kw) == SA_EINVAL, tag              # out inside in
        assert check(field, X + n_out // 2, X, **kw) == SA_EINVAL, tag             # in inside (or reaching into) out
        for off in (1, 2, 4, 8, 12, 16, 32):                                      # both pointers: 16-byte aligned
            assert check(field, BASE + off, FAR, **kw) == (SA_OK if off % 16 == 0 else SA_EINVAL), off
            assert check(field, BASE, FAR + off, **kw) == (SA_OK if off % 16 == 0 else SA_EINVAL), off
        for null in ("a_in", "a_out"):
            assert check(field=field, **kw, **{null: 0}) == SA_EINVAL, null


def test_refusals_in_their_order(check, hold_lib):
    """1 negative rows, 2 the scalar arguments and the ranks (also at rows 0), 3 rows that are no multiple of the group, 4 the
    empty call, 5 the pointers: each refusal is shown to win over every later one by making the later ones wrong too."""
    bad = [dict(field=-1), dict(field=3), dict(group=1), dict(group=0), dict(group=129), dict(group=-3), dict(group=2 ** 31 - 1),
           dict(q=0), dict(q=9), dict(q=-1), dict(ranks=None), dict(ranks=(3,)), dict(ranks=(-1,)), dict(ranks=(0, 0, 3)),
           dict(ranks=(0,) * 7 + (-1,)), dict(ranks=(2,), group=2), dict(ranks=(128,), group=128), dict(ranks=(2 ** 31 - 1,)),
           dict(ranks=(-2 ** 31,)), dict(group=1, ranks=None), dict(group=200, ranks=None, q=3)]
    wrong_ptrs = [dict(), dict(a_in=0, a_out=0), dict(a_in=BASE + 1, a_out=BASE + 3), dict(a_in=BASE, a_out=BASE)]
    # 1: before bad arguments, rows that do not divide and bad pointers
    for kw in [dict()] + bad:
        for p in wrong_ptrs:
            assert check(rows=-1, **kw, **p) == SA_ESHAPE, (kw, p)
            assert check(rows=-(1 << 31), **kw, **p) == SA_ESHAPE, (kw, p)
    # 2: before the rows that do not divide, the empty call and the pointers
    for rows in (0, 1, 5, 6, (1 << 31) - 1):
        for kw in bad:
            for p in wrong_ptrs:
                assert check(rows=rows, **kw, **p) == SA_EINVAL, (rows, kw, p)
    # 3: rows that are no multiple of the group, before the pointers
    for rows, group in ((1, 3), (5, 3), (7, 2), (129, 128), ((1 << 31) - 1, 2), ((1 << 31) - 2, 128)):
        for p in wrong_ptrs:
            assert check(rows=rows, group=group, **p) == SA_ESHAPE, (rows, group, p)
    # 4: the empty call is SA_OK whatever the pointers are
    for p in wrong_ptrs:
        for field in (0, 1, 2):
            assert check(field=field, rows=0, **p) == SA_OK, p
    # 5: the pointers, last
    for p in wrong_ptrs[1:]:
        assert check(rows=6, **p) == SA_EINVAL, p
    assert check(rows=6) == SA_OK
    # within 2: the group and q are judged before the ranks are read -- a null array with a bad group is the bad group's
    # refusal, and the same code; what shows it is that the call returns at all with q = 9 and an array of one entry (the
    # stand-alone program holds every array at exactly q entries under the address sanitizer)
    assert check(q=9, ranks=(0,)) == SA_EINVAL and check(q=8, ranks=None, group=1) == SA_EINVAL
    # the edges of every scalar that are good, and rows = 2^31 - 2: a multiple of 2 whose bytes need 64 bits
    for kw in (dict(ranks=(0,)), dict(ranks=(2,) * 8), dict(group=2, ranks=(1, 0)), dict(group=128, rows=128, ranks=(127, 0, 64)),
               dict(field=2), dict(ranks=(1, 0, 1, 2)), dict(rows=(1 << 31) - 2, group=2, a_in=1 << 20, a_out=1 << 62),
               dict(rows=(1 << 31) - 2, group=2, field=2, ranks=(0,) * 8, a_in=1 << 62, a_out=1 << 20)):
        assert check(**kw) == SA_OK, kw
    # at rows = 2^31 - 2 and group 2 the input is 2^47 - 2^17 bytes and the output, at q = 1, half of that
    big = dict(rows=(1 << 31) - 2, group=2)
    n_in, n_out = ((1 << 31) - 2) * ROW, ((1 << 30) - 1) * ROW
    assert check(a_in=1 << 20, a_out=(1 << 20) + n_in, **big) == SA_OK
    assert check(a_in=1 << 20, a_out=(1 << 20) + n_in - 16, **big) == SA_EINVAL
    assert check(a_in=(1 << 50) + n_out, a_out=1 << 50, **big) == SA_OK
    assert check(a_in=(1 << 50) + n_out - 16, a_out=1 << 50, **big) == SA_EINVAL
    assert hold_lib.sa_hold_last_error() == b""                   # the check alone leaves the thread's text alone


def test_standalone_program_under_host_sanitizers(tmp_path):
    """tests/cpp/test_sa_hold_check.cpp + csrc/sa_hold_check.cpp, host only, under the address and undefined-behaviour
    sanitizers when they link here (a plain build otherwise: the program's own checks still run): the same arithmetic at rows
    up to 2^31 - 1 and addresses near 2^47 and 2^64, every array of ranks exactly q long.  Nothing is loaded into this
    process."""
    assert standalone_checks(tmp_path, "test_sa_hold_check", ["sa_hold_check.cpp"]) > 100000


# ------------------------------------------------------------------------------------------------- the past-4-GiB shapes
@pytest.mark.parametrize("field, A, q", OFFSET_CALLS)
def test_offset_calls_are_held_to_the_rules_of_the_offset_cases(field, A, q):
    """The rules tests/test_offset_cases_cpu.py states: the last row of the deciding tensor -- a row being what belongs to one
    output row, A input rows -- starts at or beyond 2^32 with at most EXTRA rows more; the period is a multiple of A, above
    512 and no divisor of a power of two.  With q = A = 2 on magnitudes the output is as large as the input: both pass 2^32;
    on records the input rows are 128 KiB apart and the output decides."""
    P, B = offset_shape(field, A, q)
    per_group = {"in": A * ROW * (1 if field is None else 2), "out": q * ROW}
    name, row_bytes = offset_cases.deciding_tensor(per_group)
    G = B // A
    assert B % A == 0 and B % P != 0
    assert name == ("in" if field is None else "out") and row_bytes == min(per_group.values())
    assert offset_cases.last_row_start(row_bytes, G - offset_cases.EXTRA) >= offset_cases.TWO32
    assert offset_cases.last_row_start(row_bytes, G - offset_cases.EXTRA - 1) < offset_cases.TWO32
    assert P == offset_cases.period(A) and P % A == 0 and P > 512 and (P & (P - 1)) and (1 << 40) % P
    for v in per_group.values():                                  # every tensor of the call passes 2^32 too
        assert offset_cases.last_row_start(v, G) >= offset_cases.TWO32
    assert G == (32768 if field is None else 65536) + 1 + offset_cases.EXTRA
    assert hold_class(A) == 8 and hold_bins(8, field) == (4 if field is None else 2)
