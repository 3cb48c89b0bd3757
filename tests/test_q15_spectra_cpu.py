"""CPU: the full-resolution max hold and summed power over groups of A = 2^a frames (include/specan_ext.h: sa_spectra_q15,
sa_spectra_q15_p12, sa_fold_iq_q15) as far as no GPU is needed: the extension header against the built library and the second
binding table abi.EXT_SIGNATURES, the refusals of the three calls through sa_ext_check_pointers with made-up addresses (every
expected answer is worked out here from the words of the header), the same arithmetic in a stand-alone program under the host
sanitizers, and the numpy mirror frames.spectrum_of_frames against a direct evaluation."""
import ctypes
import os

import numpy as np
import pytest

from conftest import N, ROOT
from native import compiles_as_c, declared, standalone_checks

SA_OK, SA_EINVAL, SA_ESHAPE = 0, -1, -2
SPECTRA, SPECTRA_P12, FOLD = 0, 1, 2
BASE = (1 << 47) - (1 << 36)
FAR = BASE + (1 << 40)
EXT_HEADER = os.path.join(ROOT, "include", "specan_ext.h")


def in_bytes(entry, hop, B):
    if entry == FOLD:
        return B * 65536
    num, den = ((2, 1), (3, 2))[entry]
    samples = B * N if hop == 0 else (B - 1) * hop + N
    return samples * num // den


def out_bytes(log2a, B):
    return (B >> log2a) * 131072


@pytest.fixture(scope="module")
def check(hip_lib_built):
    return hip_lib_built.sa_ext_check_pointers


def test_extension_header_and_binding_table(hip_lib_built):
    """Name for name: declared in specan_ext.h = exported = bound in abi.EXT_SIGNATURES with a c_int result; nothing is in both
    tables or both headers; the version-4 surface is what it was."""
    from fpga_real_time_fft_analyzer_amd import abi
    names = declared(EXT_HEADER)
    assert names == ["sa_ext_check_pointers", "sa_ext_version", "sa_fold_iq_q15", "sa_spectra_q15", "sa_spectra_q15_p12"]
    assert sorted(abi.EXT_SIGNATURES) == names
    assert not set(abi.EXT_SIGNATURES) & set(abi.SIGNATURES)
    assert not set(names) & set(declared(os.path.join(ROOT, "include", "specan.h")))
    for name in names:
        fn, (restype, argtypes) = getattr(hip_lib_built, name), abi.EXT_SIGNATURES[name]
        assert fn.argtypes is not None and list(fn.argtypes) == list(argtypes), name
        assert fn.restype is restype is ctypes.c_int, name
    assert hip_lib_built.sa_ext_version() == abi.SA_EXT_VERSION == 1
    assert "#define SA_EXT_VERSION 1" in open(EXT_HEADER).read()
    assert abi.SA_EXT_ENTRIES == ("sa_spectra_q15", "sa_spectra_q15_p12", "sa_fold_iq_q15")
    assert len(abi.SIGNATURES) == 45 and hip_lib_built.sa_abi_version() == 4


def test_extension_header_compiles_as_c(tmp_path):
    compiles_as_c(tmp_path, '#include "specan_ext.h"\n'
                   "int use(sa_handle *h, const int16_t *x, sa_trace_point_q15 *o) { return sa_spectra_q15(h, x, o, 8, 2, 0, 0)"
                   " + sa_fold_iq_q15(h, x, o, 8, 2, 0) + sa_ext_check_pointers(SA_EXT_ENTRY_FOLD_IQ_Q15, 2, 0, 16, 32, 0)"
                   " + (SA_EXT_ENTRY_COUNT - 3) + (int)SA_Q15_HOP_STREAM_SAMPLES(8, 4096); }\n")


def test_known_answers_of_the_header(check):
    """The header's four byte counts: `out` right behind what `in` reads is accepted, 16 bytes and 1 byte earlier refused; `in`
    right behind what is written is accepted, `out` 16 bytes or 1 byte further in refused."""
    cases = ((SPECTRA, 2, 0, 8, 262144, 262144), (SPECTRA, 2, 4096, 8, 90112, 262144), (SPECTRA_P12, 2, 4096, 8, 67584, 262144),
             (FOLD, 2, 0, 8, 524288, 262144))
    assert (8 - 1) * 4096 + N == 45056
    for entry, a, hop, B, n_in, n_out in cases:
        tag = (entry, a, hop, B)
        assert (in_bytes(entry, hop, B), out_bytes(a, B)) == (n_in, n_out), tag
        assert check(entry, a, hop, BASE, BASE + n_in, B) == SA_OK, tag
        assert check(entry, a, hop, BASE, BASE + n_in - 16, B) == SA_EINVAL, tag
        assert check(entry, a, hop, BASE, BASE + n_in - 1, B) == SA_EINVAL, tag
        assert check(entry, a, hop, BASE, BASE - n_out, B) == SA_OK, tag
        assert check(entry, a, hop, BASE, BASE - n_out + 16, B) == SA_EINVAL, tag
        assert check(entry, a, hop, BASE, BASE - n_out + 1, B) == SA_EINVAL, tag
        assert check(entry, a, hop, BASE, BASE, B) == SA_EINVAL, tag
        assert check(entry, a, hop, BASE, FAR, B) == SA_OK and check(entry, a, hop, FAR, BASE, B) == SA_OK, tag


def test_overlap_is_decided_on_the_bytes_of_the_call(check):
    for entry in (SPECTRA, SPECTRA_P12, FOLD):
        for a in (1, 3, 7):
            A = 1 << a
            for hop in ((0,) if entry == FOLD else (0, 8, 4104, 16376, 16384)):
                for B in (A, 2 * A, 5 * A):
                    tag = (entry, a, hop, B)
                    n_in, n_out = in_bytes(entry, hop, B), out_bytes(a, B)
                    behind = -(-(BASE + n_in) // 16) * 16
                    assert check(entry, a, hop, BASE, behind, B) == SA_OK, tag
                    assert check(entry, a, hop, BASE, behind - 16, B) == SA_EINVAL, tag
                    if behind == BASE + n_in:
                        assert check(entry, a, hop, BASE, behind - 1, B) == SA_EINVAL, tag
                    else:
                        assert entry == SPECTRA_P12 and hop not in (0, 16384)
                    front = BASE - n_out
                    assert check(entry, a, hop, BASE, front, B) == SA_OK, tag
                    assert check(entry, a, hop, BASE, front + 16, B) == SA_EINVAL, tag
                    assert check(entry, a, hop, BASE, front + 1, B) == SA_EINVAL, tag
                    for off in (1, 2, 4, 8, 12, 16, 32):
                        want = SA_OK if off % 16 == 0 else SA_EINVAL
                        assert check(entry, a, hop, BASE + off, FAR, B) == want, tag + (off,)
                        assert check(entry, a, hop, BASE, FAR + off, B) == want, tag + (off,)
                    assert check(entry, a, hop, 0, FAR, B) == SA_EINVAL and check(entry, a, hop, BASE, 0, B) == SA_EINVAL, tag


def test_refusals_in_their_order(check):
    """1 the entry, 2 a negative batch, 3 log2a and hop (also at batch 0), 4 the empty batch, 5 the group, 6 the pointers: each
    refusal is shown to win over every later one by making the later ones wrong too."""
    for entry in (3, -1, 99):                                                        # 1: before everything
        for B in (-1, 0, 8, 9):
            assert check(entry, 2, 0, BASE, FAR, B) == SA_EINVAL
            assert check(entry, 0, 4, 0, 0, B) == SA_EINVAL
    for entry in (SPECTRA, SPECTRA_P12, FOLD):
        good_hop = 0 if entry == FOLD else 4096
        # 2: a negative batch before a bad log2a, a bad hop and bad pointers
        for a, hop in ((2, good_hop), (0, good_hop), (8, 4), (2, 12)):
            assert check(entry, a, hop, 0, 0, -1) == SA_ESHAPE, (entry, a, hop)
            assert check(entry, a, hop, BASE, FAR, -128) == SA_ESHAPE, (entry, a, hop)
        # 3: the arguments before the empty batch, the group and the pointers
        for B in (0, 8, 9, 1):
            for a in (0, 8, -1, 64):
                assert check(entry, a, good_hop, BASE, FAR, B) == SA_EINVAL, (entry, a, B)
                assert check(entry, a, good_hop, 0, 0, B) == SA_EINVAL, (entry, a, B)
            for hop in (4, 12, 4100, 16392, -8, 1 << 20):
                assert check(entry, 2, hop, BASE, FAR, B) == SA_EINVAL, (entry, hop, B)
                assert check(entry, 2, hop, 0, 0, B) == SA_EINVAL, (entry, hop, B)
            if entry == FOLD:                                                        # any hop: the fold takes frames
                for hop in (8, 4096, 16384):
                    assert check(entry, 2, hop, BASE, FAR, B) == SA_EINVAL, (hop, B)
        # 4: the empty batch is SA_OK whatever the pointers are
        for a in range(1, 8):
            for a_in, a_out in ((BASE, FAR), (0, 0), (BASE + 1, BASE + 3)):
                assert check(entry, a, good_hop, a_in, a_out, 0) == SA_OK, (entry, a)
        # 5: the batch before the pointers
        for a in (1, 3, 7):
            A = 1 << a
            for B in (1, A - 1, A + 1, 2 * A + 1, 3 * A - 1):
                if B % A:
                    assert check(entry, a, good_hop, BASE, FAR, B) == SA_ESHAPE, (entry, a, B)
                    assert check(entry, a, good_hop, 0, 0, B) == SA_ESHAPE, (entry, a, B)
                    assert check(entry, a, good_hop, BASE + 1, BASE + 3, B) == SA_ESHAPE, (entry, a, B)
        # 6: the pointers, last
        assert check(entry, 2, good_hop, 0, FAR, 8) == SA_EINVAL and check(entry, 2, good_hop, BASE, 0, 8) == SA_EINVAL
        assert check(entry, 2, good_hop, BASE, FAR, 8) == SA_OK
        # every log2a there is, every hop there is
        assert {a for a in range(-2, 12) if check(entry, a, 0, BASE, FAR, 128) == SA_OK} == set(range(1, 8))
        hops = {hop for hop in range(-16, N + 32, 4) if check(entry, 2, hop, BASE, FAR, 8) == SA_OK}
        assert hops == ({0} if entry == FOLD else {0} | set(range(8, N + 1, 8)))


def test_standalone_program_under_host_sanitizers(tmp_path):
    """tests/cpp/test_sa_ext_pointers.cpp + csrc/sa_pointers.cpp, host only, under the address and undefined-behaviour
    sanitizers when they link here (a plain build otherwise: the program's own checks still run): the same arithmetic at
    B = 70 000, B = 2^31 - 128 and addresses near 2^47 and 2^64."""
    assert standalone_checks(tmp_path, "test_sa_ext_pointers", ["sa_pointers.cpp"]) > 50000


@pytest.mark.parametrize("A", [2, 8, 128])
def test_spectrum_of_frames_against_a_direct_evaluation(A):
    """Random full-scale int16 IQ frames whose first 64 bins hold (-32768, -32768), 2^31 each, with one all-zero frame in the
    group: bin 0 sums to (A - 1) 2^31.  Power bits are those of the int64 sum converted once, peak bits the maximum of
    decode_mag_16iq_le; over buckets of W = 2 and 64 bins the records add up to (power) and top (peak) trace_of_frames's."""
    from fpga_real_time_fft_analyzer_amd import frames
    rng = np.random.default_rng(1400 + A)
    iq = rng.integers(-32768, 32768, size=(A, N, 2)).astype("<i2")
    iq[:, :64] = -32768
    iq[A // 2] = 0
    fb = [f.tobytes() for f in iq]
    peak, power, exact = frames.spectrum_of_frames(fb)
    re, im = iq[..., 0].astype(np.int64), iq[..., 1].astype(np.int64)
    want = (re * re + im * im).sum(axis=0)
    assert exact.dtype == np.int64 and exact.shape == (N,) and np.array_equal(exact, want)
    assert exact[0] == (A - 1) << 31
    assert power.dtype == np.float32 and np.array_equal(power.view(np.uint32), want.astype(np.float32).view(np.uint32))
    mag = np.stack([frames.decode_mag_16iq_le(f) for f in fb])
    assert peak.dtype == np.float32 and np.array_equal(peak.view(np.uint32), mag.max(axis=0).view(np.uint32))
    if A >= 8:
        assert (power.astype(np.float64) != want).any()                              # the rounding is a real one somewhere
    for W in (2, 64):
        tp, _, te = frames.trace_of_frames(fb, W)
        assert np.array_equal(exact.reshape(-1, W).sum(axis=1), te), W
        assert np.array_equal(peak.reshape(-1, W).max(axis=1).view(np.uint32), tp.view(np.uint32)), W


def test_spectrum_of_frames_edges():
    from fpga_real_time_fft_analyzer_amd import frames
    z = frames.spectrum_of_frames([bytes(65536)] * 4)
    assert not z[0].view(np.uint32).any() and not z[1].view(np.uint32).any() and not z[2].any()
    full = np.full((N, 2), -32768, "<i2").tobytes()
    _, power, exact = frames.spectrum_of_frames([full] * 128)
    assert (exact == 1 << 38).all() and (power == np.float32(2.0 ** 38)).all()       # the largest sum there is
    for bad in ([bytes(65536)], [bytes(65536)] * 3, [bytes(65536)] * 256):
        with pytest.raises(ValueError):
            frames.spectrum_of_frames(bad)
    with pytest.raises(ValueError):
        frames.spectrum_of_frames([bytes(65535)] * 2)
    for bad in (1, True):                                                            # the bucketed mirror keeps refusing W = 1
        with pytest.raises(ValueError):
            frames.trace_of_frames([bytes(65536)] * 2, bad)


def test_the_wrappers_surface():
    """The Python entry points exist beside the pinned tables, which are what they were."""
    from fpga_real_time_fft_analyzer_amd import chain
    assert callable(chain.SpectrumChain.spectra_q15) and callable(chain.SpectrumChain.fold_iq_q15)
    assert sorted(chain._ARGS) == ["sa_filter_q15", "sa_filter_q15_p12", "sa_process_f32", "sa_process_f32_i16", "sa_process_f32_p12",
                                   "sa_process_q15", "sa_process_q15_out", "sa_process_q15_p12"]
    assert not any(isinstance(k, tuple) and 1 in k for k in chain.Q15_TRACE_AVG_CHAIN.outputs) and 1 not in chain.Q15_TRACE_CHAIN.outputs
    for bad in (0, 1, 3, 256, 2.0, True, None, "4"):
        with pytest.raises(chain.SpecanError) as e:
            chain.SpectrumChain._log2_group(bad)
        assert e.value.code == SA_EINVAL, bad
    assert [chain.SpectrumChain._log2_group(g) for g in chain.TRACE_GROUPS] == list(range(1, 8))
