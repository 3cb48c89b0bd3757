"""CPU: the packed 12-bit input of the integer chain (sa_process_q15_p12, sa_filter_q15_p12) as far as it can be checked
without a GPU: the two symbols and their ctypes signatures, and numpy models of the two address maps by which the kernels
find a sample in the packed frame -- the 12-byte unit of the window kernel and the cascades' staging waves
(cascade_q15.hip, q15_load_tile) and stage 0 of the FFT (fft_q15.hip, fx_load16).  Each model is enumerated over a whole
frame, must reproduce ingest.unpack12 on random bytes (every bit pattern is a valid frame) and must stay inside the frame."""
import ctypes as C
import os
import re

import numpy as np

from conftest import N, ROOT

P12 = 24576
FRAME_DWORDS = P12 // 4


def packed_frame(seed):
    return np.random.default_rng(seed).integers(0, 256, P12, dtype=np.uint8)


def sext12(v):
    v = np.asarray(v, np.int64) & 0xFFF
    return (v - ((v & 0x800) << 1)).astype(np.int16)


def test_library_exports_both_symbols(hip_lib_built):
    txt = open(os.path.join(ROOT, "include", "specan.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("sa_process_q15_p12", "sa_filter_q15_p12"):
        assert re.search(r"\b%s\s*\(" % name, txt), f"{name} not declared in include/specan.h"
        assert hasattr(hip_lib_built, name), f"{name} not exported"
    assert hip_lib_built.sa_abi_version() == 4


def test_abi_py_carries_the_signatures(hip_lib_built):
    H = C.c_void_p
    assert hip_lib_built.sa_process_q15_p12.argtypes == [H, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    assert hip_lib_built.sa_filter_q15_p12.argtypes == [H, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    assert hip_lib_built.sa_process_q15_p12.restype is C.c_int and hip_lib_built.sa_filter_q15_p12.restype is C.c_int
    # same shape as the int16 entry points they stand beside
    assert hip_lib_built.sa_process_q15_p12.argtypes == hip_lib_built.sa_process_q15_out.argtypes
    assert hip_lib_built.sa_filter_q15_p12.argtypes == hip_lib_built.sa_filter_q15.argtypes


def test_null_handle_is_rejected_without_a_gpu(hip_lib_built):
    from fpga_real_time_fft_analyzer_amd.abi import SA_EINVAL
    assert hip_lib_built.sa_process_q15_p12(None, None, None, 1, 0, None) == SA_EINVAL
    assert hip_lib_built.sa_filter_q15_p12(None, None, None, 1, None) == SA_EINVAL


def test_fft_stage0_address_map():
    """fx_load16(SaP12): thread t, m = 0..15 takes sample t + 1024 m from dword (12 t >> 5) + 384 m at bit 12 t & 31; the
    second dword is the next one only where the sample straddles (shift > 20) and the first again elsewhere; funnel shift
    and sign-extending extract of 12 bits."""
    from fpga_real_time_fft_analyzer_amd.ingest import unpack12
    t = np.arange(1024)[:, None]
    m = np.arange(16)[None, :]
    bit = 12 * t
    sh = bit & 31
    i0 = (bit >> 5) + 384 * m
    straddle = sh > 20
    i1 = i0 + straddle
    # the straddle rule and the shift do not depend on m
    assert np.array_equal(straddle[:, 0], np.isin(t[:, 0] % 8, (2, 5)))
    assert np.array_equal(np.unique(sh[straddle[:, 0]]), [24, 28])
    # never outside the frame -- and not by luck: the dword after the first would be, for the frame's last two samples
    assert i0.min() == 0 and i0.max() == FRAME_DWORDS - 1 and i1.max() == FRAME_DWORDS - 1
    over = np.argwhere(i0 + 1 > FRAME_DWORDS - 1)
    assert sorted(map(tuple, over)) == [(1022, 15), (1023, 15)] and not straddle[1022:].any()
    for seed in (1, 2):
        p = packed_frame(seed)
        d = p.view("<u4").astype(np.uint64)
        lo, hi = d[i0], d[i1]
        v = (((hi << np.uint64(32)) | lo) >> sh.astype(np.uint64)) & np.uint64(0xFFFFFFFF)       # v_alignbit_b32
        got = np.empty(N, np.int16)
        got[(t + 1024 * m).ravel()] = sext12(v).ravel()                                           # v_bfe_i32 .., 0, 12
        assert np.array_equal(got, unpack12(p))


def test_tile_unit_address_map():
    """q15_load_tile / window_q15_kernel<SaP12>: samples 8 u .. 8 u + 7 are the 12 bytes at byte 3 (8 u) / 2 = 12 u, three
    aligned dwords that end with the frame at the latest; p12_unpack8 takes them apart."""
    from fpga_real_time_fft_analyzer_amd.ingest import unpack12
    u = np.arange(N // 8)
    byte = 3 * (8 * u) // 2
    assert np.array_equal(byte, 12 * u) and not (byte % 4).any() and byte.max() + 12 == P12
    for seed in (3, 4):
        p = packed_frame(seed)
        d = p.view("<u4").astype(np.uint64)
        w0, w1, w2 = d[byte // 4], d[byte // 4 + 1], d[byte // 4 + 2]
        align = lambda h, l, s: (((h << np.uint64(32)) | l) >> np.uint64(s)) & np.uint64(0xFFFFFFFF)
        s8 = [w0, w0 >> np.uint64(12), align(w1, w0, 24), w1 >> np.uint64(4), w1 >> np.uint64(16), align(w2, w1, 28),
              w2 >> np.uint64(8), w2 >> np.uint64(20)]
        got = np.stack([sext12(x) for x in s8], axis=1).reshape(N)
        assert np.array_equal(got, unpack12(p))
