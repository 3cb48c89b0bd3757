"""Shared by the GPU tests of the integer chain's output kinds (a plain module, like gpu_support.py): the numpy mirrors of
what the FFT epilogues and the two fold kernels compute, applied to [B,N,2] int16 IQ frames -- the oracle's, or the handle's
own IQ output where a test has held that to the oracle first.  Every one of them is exact: magnitudes through
frames.decode_mag_16iq_le (the committed mirror of gui.py:250-260), powers as int64 sums rounded ONCE to float32 (nearest
even; tests/test_q15_trace_cpu.py and tests/test_q15_trace_avg_cpu.py pin that conversion)."""
import numpy as np

from conftest import N


def bits(a):
    """float32 values as their bit patterns: comparisons are by bits (+0.0 is not -0.0, a NaN equals itself)"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def decode(iq):
    """[B,N,2] int16 frames -> (mag float32 [B,N] through frames.decode_mag_16iq_le, integer power int64 [B,N])"""
    from fpga_real_time_fft_analyzer_amd import frames
    iq = np.ascontiguousarray(iq).astype("<i2", copy=False)
    mag = np.stack([frames.decode_mag_16iq_le(iq[f].tobytes()) for f in range(iq.shape[0])])
    return mag, iq[..., 0].astype(np.int64) ** 2 + iq[..., 1].astype(np.int64) ** 2


def marker_expect(mag, ip, lo, hi):
    """SA_Q15_OUT_MARKER over the bins [lo, hi): (peak_mag float32 [B], peak_bin int32 [B] -- the lowest bin attaining the
    peak --, band_power int64 [B]) of decoded frames"""
    sl = mag[:, lo:hi]
    return sl.max(axis=1), (lo + sl.argmax(axis=1)).astype(np.int32), ip[:, lo:hi].sum(axis=1)


def marker_records(rec):
    """[B,4] int32 record array or tensor -> (peak_mag f32, peak_bin i32, band_power i64) numpy arrays"""
    r = np.ascontiguousarray(rec if isinstance(rec, np.ndarray) else rec.cpu().numpy())
    return r[:, 0].copy().view(np.float32), r[:, 1].copy(), r.view(np.int64)[:, 1].copy()


def trace_expect(mag, ip, W, A=1):
    """SA_Q15_TRACE_KIND / SA_Q15_TRACE_AVG_KIND: (peak float32 [B/A,P], power float32 [B/A,P], exact int64 [B/A,P]) of decoded
    frames, over buckets of W bins and groups of A consecutive frames (P = N / W)"""
    B = mag.shape[0]
    assert B % A == 0
    exact = ip.reshape(B // A, A, N // W, W).sum(axis=(1, 3))
    return mag.reshape(B // A, A, N // W, W).max(axis=(1, 3)), exact.astype(np.float32), exact


def spectra_expect(mag, ip, A):
    """sa_spectra_q15: (peak float32 [B/A,N], power float32 [B/A,N], exact int64 [B/A,N]) of decoded frames, per bin over
    groups of A consecutive frames"""
    B = mag.shape[0]
    assert B % A == 0
    exact = ip.reshape(B // A, A, N).sum(axis=1)
    return mag.reshape(B // A, A, N).max(axis=1), exact.astype(np.float32), exact
