"""CPU: the fold of float magnitudes over groups of A = 2^a frames and buckets of W = 2^k bins (include/specan_fold.h:
sa_fold_mag_f32 of libspecan_fold.so; SpectrumChain.fold_mag_f32 and spectra_f32) as far as no GPU is needed: the header against
the built library and the third binding table abi.FOLD_SIGNATURES, the kernels the library holds, the refusals through
sa_fold_check with made-up addresses (every expected answer is worked out here from the words of the header), the same
arithmetic in a stand-alone program under the host sanitizers, and the numpy mirror frames.fold_of_mags against order probes
whose expected bits are derived by hand below, never from the code under test."""
import ctypes
import os

import numpy as np
import pytest

from conftest import N
from kernel_inventory import TABLE, inventory, lds_of, lds_remarks, unit_text
from native import INCLUDE, compiles_as_c, declared, exported, standalone_checks
from reduction_libraries import BASE, SA_EINVAL, SA_ESHAPE, SA_OK, bits, built

FAR = BASE + (1 << 40)
HEADER = os.path.join(INCLUDE, "specan_fold.h")
NAMES = ["sa_fold_check", "sa_fold_last_error", "sa_fold_mag_f32", "sa_fold_version"]
PAIRS = [(a, k) for a in range(8) for k in range(7) if (a, k) != (0, 0)]


def in_bytes(B):
    return B * 65536


def out_bytes(a, k, B):
    return (B >> a) * (N >> k) * 8


def bits1(x):
    """the bits of one value"""
    return int(bits(x).ravel()[0])


def f32(*v):
    return np.array(v, np.float32)


@pytest.fixture(scope="module")
def fold_lib():
    return built("fold")


@pytest.fixture(scope="module")
def check(fold_lib):
    return fold_lib.sa_fold_check


# ------------------------------------------------------------------------------------------------------------ the surface
def test_header_library_and_binding_table(fold_lib):
    """Name for name: declared in specan_fold.h = exported by libspecan_fold.so = bound in abi.FOLD_SIGNATURES, each with a
    c_int result except the error text; nothing is in the other two tables or headers, which are what they were."""
    from fpga_real_time_fft_analyzer_amd import abi
    assert declared(HEADER) == NAMES
    assert [n for n in exported(abi.FOLD_LIB_PATH) if "sa_" in n] == NAMES
    assert sorted(abi.FOLD_SIGNATURES) == NAMES
    assert not set(NAMES) & (set(abi.SIGNATURES) | set(abi.EXT_SIGNATURES))
    assert not set(NAMES) & set(declared(os.path.join(INCLUDE, "specan.h")) + declared(os.path.join(INCLUDE, "specan_ext.h")))
    for name in NAMES:
        fn, (restype, argtypes) = getattr(fold_lib, name), abi.FOLD_SIGNATURES[name]
        assert fn.argtypes is not None and list(fn.argtypes) == list(argtypes), name
        assert fn.restype is restype is (ctypes.c_char_p if name == "sa_fold_last_error" else ctypes.c_int), name
    assert fold_lib.sa_fold_version() == abi.SA_FOLD_VERSION == 1
    assert "#define SA_FOLD_VERSION 1" in open(HEADER).read()
    assert fold_lib.sa_fold_last_error() == b""
    assert len(abi.SIGNATURES) == 45 and len(abi.EXT_SIGNATURES) == 5
    assert os.path.basename(abi.FOLD_LIB_PATH) == "libspecan_fold.so" and os.path.dirname(abi.FOLD_LIB_PATH) == os.path.dirname(abi.LIB_PATH)


def test_header_compiles_as_c(tmp_path):
    compiles_as_c(tmp_path, '#include "specan_fold.h"\n'
                   "int use(const float *m, sa_fold_point *o) { return sa_fold_mag_f32(m, o, 8, 2, 4, 0) + sa_fold_check(2, 4, 16, 32, 0)"
                   " + sa_fold_version() - SA_FOLD_VERSION + (int)sizeof(sa_fold_point) - 8 + (sa_fold_last_error()[0] != 0)"
                   " + SA_N - 16384 + SA_FOLD_LOG2A_MAX - 7 + SA_FOLD_LOG2W_MAX - 6; }\n")


def test_kernel_inventory(fold_lib):
    """The library holds the seven instantiations and nothing else; none uses LDS, static (the compiler's remark, one figure
    per instantiation) or dynamic (no declaration in the unit or its headers); libspecan_hip.so holds what it held."""
    from fpga_real_time_fft_analyzer_amd import abi
    assert inventory(abi.FOLD_LIB_PATH) == {f"fold_mag_f32_kernel<{k}>" for k in range(7)}
    assert lds_of(lds_remarks("fold_mag_f32.hip"), "fold_mag_f32_kernel") == [0] * 7
    assert "extern __shared__" not in unit_text("fold_mag_f32.hip") and "__shared__" not in unit_text("fold_mag_f32.hip")
    if not os.path.exists(abi.LIB_PATH):
        abi.build()
    assert inventory(abi.LIB_PATH) == set(TABLE)


# -------------------------------------------------------------------------------------------------------------- the check
def test_known_answers_of_the_header(check):
    """The header's three cases: `out` right behind what `mag` reads is accepted, 16 bytes and 1 byte earlier refused; `mag`
    right behind what is written is accepted, `out` 16 bytes or 1 byte further in refused."""
    for a, k, B, n_in, n_out in ((2, 0, 8, 524288, 262144), (0, 4, 8, 524288, 65536), (4, 4, 16, 1048576, 8192)):
        tag = (a, k, B)
        assert (in_bytes(B), out_bytes(a, k, B)) == (n_in, n_out), tag
        assert check(a, k, BASE, BASE + n_in, B) == SA_OK, tag
        assert check(a, k, BASE, BASE + n_in - 16, B) == SA_EINVAL, tag
        assert check(a, k, BASE, BASE + n_in - 1, B) == SA_EINVAL, tag
        assert check(a, k, BASE, BASE - n_out, B) == SA_OK, tag
        assert check(a, k, BASE, BASE - n_out + 16, B) == SA_EINVAL, tag
        assert check(a, k, BASE, BASE - n_out + 1, B) == SA_EINVAL, tag
        assert check(a, k, BASE, BASE, B) == SA_EINVAL, tag
        assert check(a, k, BASE, FAR, B) == SA_OK and check(a, k, FAR, BASE, B) == SA_OK, tag


def test_overlap_and_alignment_for_every_pair(check):
    for a, k in PAIRS:
        A = 1 << a
        for B in (A, 5 * A):
            tag = (a, k, B)
            n_in, n_out = in_bytes(B), out_bytes(a, k, B)
            assert n_out % 16 == 0, tag
            assert check(a, k, BASE, BASE + n_in, B) == SA_OK, tag
            assert check(a, k, BASE, BASE + n_in - 16, B) == SA_EINVAL, tag
            front = BASE - n_out
            assert check(a, k, BASE, front, B) == SA_OK, tag
            assert check(a, k, BASE, front + 16, B) == SA_EINVAL, tag
            for off in (1, 2, 4, 8, 12, 16, 32):
                want = SA_OK if off % 16 == 0 else SA_EINVAL
                assert check(a, k, BASE + off, FAR, B) == want, tag + (off,)
                assert check(a, k, BASE, FAR + off, B) == want, tag + (off,)
            assert check(a, k, 0, FAR, B) == SA_EINVAL and check(a, k, BASE, 0, B) == SA_EINVAL, tag


def test_refusals_in_their_order(check):
    """1 a negative batch, 2 log2a and log2w (also at batch 0), 3 the empty batch, 4 the group and the launch bound, 5 the
    pointers: each refusal is shown to win over every later one by making the later ones wrong too."""
    bad_pairs = ((0, 0), (8, 2), (-1, 2), (2, 7), (2, -1), (64, 64))
    # 1: before bad arguments, a bad group and bad pointers
    for a, k in ((2, 4),) + bad_pairs:
        assert check(a, k, 0, 0, -1) == SA_ESHAPE, (a, k)
        assert check(a, k, BASE + 1, BASE + 3, -128) == SA_ESHAPE, (a, k)
    # 2: before the empty batch, the group, the launch bound and the pointers
    for B in (0, 8, 9, 1, (1 << 31) - 1):
        for a, k in bad_pairs:
            assert check(a, k, BASE, FAR, B) == SA_EINVAL, (a, k, B)
            assert check(a, k, 0, 0, B) == SA_EINVAL, (a, k, B)
    # 3: the empty batch is SA_OK whatever the pointers are
    for a, k in PAIRS:
        for a_in, a_out in ((BASE, FAR), (0, 0), (BASE + 1, BASE + 3), (BASE, BASE)):
            assert check(a, k, a_in, a_out, 0) == SA_OK, (a, k)
    # 4: the batch before the pointers
    for a in (1, 3, 7):
        A = 1 << a
        for B in (1, A - 1, A + 1, 2 * A + 1, 3 * A - 1):
            if B % A:
                for ptrs in ((BASE, FAR), (0, 0), (BASE + 1, BASE + 3), (BASE, BASE)):
                    assert check(a, 4, *ptrs, B) == SA_ESHAPE, (a, B)
    # ... and the launch: 16 workgroups of 256 threads x 4 bins per group of frames, at most 2^31 - 1 of them
    for a in range(4):
        over, under = (1 << 27) << a, ((1 << 27) - 1) << a
        for ptrs in ((1 << 20, 1 << 62), (0, 0), (BASE + 1, BASE + 3)):
            assert check(a, 6, *ptrs, over) == SA_ESHAPE, a
        assert check(a, 6, 1 << 62, 1 << 20, under) == SA_OK, a                  # 2^43 bytes read from 2^62 on: disjoint
        assert check(a, 6, 0, 1 << 20, under) == SA_EINVAL, a
    # 5: the pointers, last
    assert check(2, 4, 0, FAR, 8) == SA_EINVAL and check(2, 4, BASE, 0, 8) == SA_EINVAL
    assert check(2, 4, BASE, FAR, 8) == SA_OK
    # every (log2a, log2w) there is
    ok = {(a, k) for a in range(-2, 12) for k in range(-2, 12) if check(a, k, BASE, FAR, 128) == SA_OK}
    assert ok == set(PAIRS) and len(ok) == 55


def test_standalone_program_under_host_sanitizers(tmp_path):
    """tests/cpp/test_sa_fold_check.cpp + csrc/sa_fold_check.cpp, host only, under the address and undefined-behaviour
    sanitizers when they link here (a plain build otherwise: the program's own checks still run): the same arithmetic at
    B = 70 000, B = 2^31 - 128 and addresses near 2^47 and 2^64."""
    assert standalone_checks(tmp_path, "test_sa_fold_check", ["sa_fold_check.cpp"]) > 50000


# ------------------------------------------------------------------------------------------------------------- the mirror
# the eight values of the order probes: squares 1, 2^-24, 0, 0 and four times 2^-54.  In float64 (ulp 2^-52 at 1) 2^-54 added
# to 1 + 2^-24 is a quarter of an ulp and vanishes, while the four of them added to each other first make 2^-52, one ulp.
# 1 + 2^-24 is the tie between the float32 values 1 and 1 + 2^-23 and goes to the even one, 0x3F800000; anything above it
# goes up, 0x3F800001.
PROBE = f32(1.0, 2.0 ** -12, 0.0, 0.0, 2.0 ** -27, 2.0 ** -27, 2.0 ** -27, 2.0 ** -27)


def test_order_across_bins_is_the_pair_tree():
    from fpga_real_time_fft_analyzer_amd import frames
    peak, power, s = frames.fold_of_mags(PROBE.reshape(1, 8), 1, 8)
    # the tree: (1 + 2^-24) + (0 + 0) = 1 + 2^-24; (2^-54 + 2^-54) + (2^-54 + 2^-54) = 2^-52; together 1 + 2^-24 + 2^-52, exact
    assert s.shape == (1, 1) and s[0, 0] == 1.0 + 2.0 ** -24 + 2.0 ** -52
    assert bits(power)[0, 0] == 0x3F800001 and bits(peak)[0, 0] == 0x3F800000
    seq = np.float64(0.0)
    for m in PROBE:                                                              # this test's own sequential sum over the bins
        seq = seq + np.float64(m) * np.float64(m)
    assert seq == 1.0 + 2.0 ** -24 and bits1(seq) == 0x3F800000


def test_order_across_frames_is_sequential_and_ascending():
    from fpga_real_time_fft_analyzer_amd import frames
    mag = np.zeros((8, 4), np.float32)
    mag[:, 1] = PROBE                                                            # the eight values as the frames of bin 1
    peak, power, s = frames.fold_of_mags(mag, 8, 1)
    assert s[0, 1] == 1.0 + 2.0 ** -24 and bits(power)[0, 1] == 0x3F800000       # each 2^-54 vanishes on arrival
    assert bits(peak)[0].tolist() == [0, 0x3F800000, 0, 0] and not bits(power)[0, [0, 2, 3]].any()
    sq = PROBE.astype(np.float64) ** 2
    desc = np.float64(0.0)
    for v in sq[::-1]:
        desc = desc + v
    pair = ((sq[0] + sq[1]) + (sq[2] + sq[3])) + ((sq[4] + sq[5]) + (sq[6] + sq[7]))
    assert bits1(desc) == bits1(pair) == 0x3F800001        # what another order would give
    # the same frames reversed: the order is that of the frame index, not of the values
    _, power_r, _ = frames.fold_of_mags(mag[::-1], 8, 1)
    assert bits(power_r)[0, 1] == 0x3F800001


def test_frames_are_summed_before_bins():
    """A = 2, W = 4: frame 0 = (1, 0, 2^-27, 2^-27), frame 1 = (2^-12, 0, 2^-27, 2^-27).  As specified, per bin over the frames
    first: c = (1 + 2^-24, 0, 2^-53, 2^-53), tree (c0 + c1) + (c2 + c3) = 1 + 2^-24 + 2^-52 -> 0x3F800001.  Bins first: frame 0
    is (1 + 0) + 2^-53, a tie that goes to the even 1; frame 1 is 2^-24 + 2^-53, exact; their sum 1 + 2^-24 + 2^-53 is again
    a tie and goes to the even 1 + 2^-24 -> 0x3F800000."""
    from fpga_real_time_fft_analyzer_amd import frames
    mag = f32(1.0, 0.0, 2.0 ** -27, 2.0 ** -27, 2.0 ** -12, 0.0, 2.0 ** -27, 2.0 ** -27).reshape(2, 4)
    _, power, s = frames.fold_of_mags(mag, 2, 4)
    assert s[0, 0] == 1.0 + 2.0 ** -24 + 2.0 ** -52 and bits(power)[0, 0] == 0x3F800001
    sq = mag.astype(np.float64) ** 2
    per_frame = [(f[0] + f[1]) + (f[2] + f[3]) for f in sq]
    assert per_frame[0] == 1.0 and per_frame[1] == 2.0 ** -24 + 2.0 ** -53
    assert bits1((np.float64(0.0) + per_frame[0]) + per_frame[1]) == 0x3F800000


def test_float32_accumulation_differs():
    from fpga_real_time_fft_analyzer_amd import frames
    rng = np.random.default_rng(1501)
    mag = np.exp(rng.uniform(-20.0, 20.0, size=(16, 1024))).astype(np.float32)
    _, power, s = frames.fold_of_mags(mag, 16, 16)
    acc = np.zeros(1024, np.float32)
    for f in mag:
        acc = acc + f * f
    while acc.shape[0] > 64:
        acc = acc[0::2] + acc[1::2]
    assert (bits(acc) != bits(power[0])).any()
    direct = (mag.astype(np.float64) ** 2).reshape(16, 64, 16).sum(axis=(0, 2))
    assert np.abs(s[0] - direct).max() <= 1e-13 * direct.max()                   # and the float64 one is a float64 sum


def test_denormals_overflow_zero_nan_and_inf():
    from fpga_real_time_fft_analyzer_amd import frames
    z = np.zeros((2, 8), np.float32)
    mag = z.copy()
    mag[0, 0] = 2.0 ** -70                                                       # power 2^-140 = 2^9 x 2^-149: a float32 denormal
    mag[0, 2] = 2.0 ** -140                                                      # a denormal input: bits 2^9; its square is 0 in float32
    mag[0, 4] = 3e38                                                             # 9e76 is past float32: +inf, the peak stays finite
    mag[0, 6] = -0.0
    assert bits(mag)[0, 2] == 0x200 and bits(mag)[0, 6] == 0x80000000
    peak, power, s = frames.fold_of_mags(mag, 1, 2)
    assert bits(peak)[0].tolist() == [(127 - 70) << 23, 0x200, bits1(3e38), 0]
    assert bits(power)[0].tolist() == [0x200, 0, 0x7F800000, 0]
    assert s[0, 1] == 2.0 ** -280 and np.isfinite(s[0, 2])
    assert not bits(peak)[1].any() and not bits(power)[1].any()                  # (+0, +0)
    # a NaN frame or a +inf frame in group 0 of 2 changes group 0 only
    rng = np.random.default_rng(1502)
    base = np.exp(rng.uniform(-60.0, 60.0, size=(4, 64))).astype(np.float32)
    clean = frames.fold_of_mags(base, 2, 4)
    for bad, top in ((np.nan, None), (np.inf, 0x7F800000)):
        m = base.copy()
        m[1] = bad
        peak, power, _ = frames.fold_of_mags(m, 2, 4)
        assert np.array_equal(bits(peak)[1], bits(clean[0])[1]) and np.array_equal(bits(power)[1], bits(clean[1])[1])
        if top is None:
            assert np.isnan(peak[0]).all() and np.isnan(power[0]).all()
            assert (bits(peak)[0] == (bits1(np.nan) & 0x7FFFFFFF)).all()
        else:
            assert (bits(peak)[0] == top).all() and (bits(power)[0] == top).all()
    m = base.copy()
    m[0, 5], m[1, 6] = np.nan, np.inf                                            # a NaN beats +inf in the record they share
    peak, power, _ = frames.fold_of_mags(m, 2, 4)
    assert np.isnan(peak[0, 1]) and np.isnan(power[0, 1]) and np.isfinite(peak[0, 0]) and np.isfinite(peak[0, 2])
    for bad in ((1, 1), (3, 1), (256, 1), (2.0, 2), (True, 2), (2, 128), (2, 3), (2, True), (None, 2)):
        with pytest.raises(ValueError):
            frames.fold_of_mags(base, *bad)
    with pytest.raises(ValueError):
        frames.fold_of_mags(base[:3], 2, 1)
    with pytest.raises(ValueError):
        frames.fold_of_mags(base.astype(np.float64), 2, 1)


def test_consistency_between_bucket_widths_and_with_numpy_max():
    from fpga_real_time_fft_analyzer_amd import frames
    rng = np.random.default_rng(1503)
    mag = np.exp(rng.uniform(-60.0, 60.0, size=(128, 256))).astype(np.float32)
    for A in (2, 4, 8, 16, 32, 64, 128):                                         # A = 1 at W = 1 is refused: below at W > 1
        p1, _, s1 = frames.fold_of_mags(mag, A, 1)
        assert np.array_equal(bits(p1), bits(mag.reshape(128 // A, A, 256).max(axis=1))), A
        for W in (2, 4, 8, 16, 32, 64):
            p, pw, s = frames.fold_of_mags(mag, A, W)
            assert np.array_equal(bits(p), bits(p1.reshape(128 // A, 256 // W, W).max(axis=2))), (A, W)
            t = s1
            while t.shape[1] > 256 // W:
                t = t[:, 0::2] + t[:, 1::2]
            with np.errstate(over="ignore"):                                     # squares past float32 round to +inf
                assert np.array_equal(t, s) and np.array_equal(bits(pw), bits(t.astype(np.float32))), (A, W)
    for W in (2, 64):                                                            # A = 1: the buckets of single frames
        p, _, _ = frames.fold_of_mags(mag, 1, W)
        assert np.array_equal(bits(p), bits(mag.reshape(128, 256 // W, W).max(axis=2))), W


# ----------------------------------------------------------------------------------------------------------- the wrappers
def test_the_wrappers_surface():
    """The Python entry points exist beside the pinned tables; a bad ``group`` or ``bucket`` is SA_EINVAL before anything of the
    object or of a library is touched (the object here has neither)."""
    from fpga_real_time_fft_analyzer_amd import chain
    cls = chain.SpectrumChain
    assert callable(cls.fold_mag_f32) and callable(cls.spectra_f32)
    assert len(chain._ARGS) == 8 and chain.TRACE_GROUPS == (2, 4, 8, 16, 32, 64, 128)
    assert chain.FOLD_GROUPS == (1, 2, 4, 8, 16, 32, 64, 128) and chain.FOLD_BUCKETS == (1, 2, 4, 8, 16, 32, 64)
    bare = object.__new__(cls)
    bad = [(g, 4) for g in (0, 3, 256, -2, 2.0, True, None, "4")] + [(4, b) for b in (0, 3, 128, -2, 2.0, True, None, "4")] + [(1, 1)]
    for group, bucket in bad:
        for call in (lambda: cls._log2_fold(group, bucket), lambda: bare.fold_mag_f32(None, group, bucket),
                     lambda: bare.spectra_f32(None, group, bucket)):
            with pytest.raises(chain.SpecanError) as e:
                call()
            assert e.value.code == SA_EINVAL, (group, bucket)
    assert [cls._log2_fold(g, 2)[0] for g in chain.FOLD_GROUPS] == list(range(8))
    assert [cls._log2_fold(2, b)[1] for b in chain.FOLD_BUCKETS] == list(range(7))
    assert cls._log2_fold(np.int64(1), 64) == (0, 6) and cls._log2_fold(128, np.int32(1)) == (7, 0)
