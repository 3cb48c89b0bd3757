"""Shared by tests/test_plan_conditioning.py (CPU) and tests/test_gpu_f32_structured.py (GPU): the per-bin spectrum
norm, the float32-FFT yardstick it is bounded by, and the cascades whose kernel variants the GPU tests reach.

The parity tests of tests/test_gpu_f32.py divide a frame's worst error by the frame's PEAK.  On a tone frame under the
Hann window the bins away from the tone sit ~1e-3 below that peak, so a defect confined to them is scaled down a
thousandfold before it meets the gate.  The per-bin norm divides by the RMS of the reference spectrum instead, and the
structured tests feed impulses, exact-bin cosines and white noise, whose spectra have no such hiding place."""
import numpy as np
from scipy import signal

N = 16384
H = N // 2 + 1


def bin_norm(got, ref):
    """max over frames of  max_k |got_k - ref_k| / RMS_k |ref_k|  (rows are frames)."""
    got = np.asarray(got).reshape(-1, np.shape(ref)[-1]).astype(np.complex128)
    ref = np.asarray(ref).reshape(got.shape).astype(np.complex128)
    rms = np.sqrt(np.mean(np.abs(ref) ** 2, axis=1))
    return float((np.abs(got - ref).max(axis=1) / np.maximum(rms, 1e-300)).max())


def peak_norm(got, ref):
    """max over frames of  max_k |got_k - ref_k| / max_k |ref_k|: the norm of the existing parity tests."""
    got = np.asarray(got).reshape(-1, np.shape(ref)[-1]).astype(np.complex128)
    ref = np.asarray(ref).reshape(got.shape).astype(np.complex128)
    return float((np.abs(got - ref).max(axis=1) / np.maximum(np.abs(ref).max(axis=1), 1e-300)).max())


def f32_fft_figure(xw32, ref):
    """bin_norm of scipy's float32 rfft of the float32 time series `xw32` against the float64 reference spectrum."""
    import scipy.fft
    return bin_norm(scipy.fft.rfft(np.asarray(xw32, np.float32), axis=-1), ref)


def fft_bound(xw32, ref):
    """The bound of a float32 FFT stage: max(1e-6, 4 x what scipy's float32 rfft achieves on the same input)."""
    return max(1e-6, 4.0 * f32_fft_figure(xw32, ref))


def real_pair(p1, p2, gain=None):
    """One section with real poles p1, p2 and the numerator b0 alone, scaled to unit DC gain."""
    g = (1 - p1) * (1 - p2) if gain is None else gain
    return np.array([[g, 0.0, 0.0, 1.0, -(p1 + p2), p1 * p2]])


def smoother_f32(p):
    """Critically damped smoother [(1-p)^2, 0, 0, 1, -2p, p^2] with its taps rounded to float32 (what
    sa_load_sos_f32 receives), widened back to float64."""
    return np.array([[(1 - p) ** 2, 0, 0, 1, -2 * p, p * p]], np.float32).astype(np.float64)


def _rtl6():
    a = [14 / 128, 0, -14 / 128, 1, 21 / 128, 107 / 128]
    b = [15 / 128, 0, -15 / 128, 1, -21 / 128, 107 / 128]
    return np.array([a, b, a, b, a, b])


def cascades():
    """name -> a0-normalised SOS.  The GPU cascade tests run every one of them; test_plan_conditioning pins which
    kernel variant each reaches (CASCADE_VARIANTS)."""
    b8 = signal.butter(8, 0.1, output="sos")
    return {
        "butter12": signal.butter(12, 0.2, output="sos"),             # 6 sections, unit-numerator form
        "rtl_default": _rtl6(),                                       # 6 sections, b2 = -b0: general form
        "long_memory": signal.butter(4, 0.002, output="sos"),         # 2 sections, no scan level skipped
        "butter3_first_order": signal.butter(3, 0.3, output="sos"),   # a first-order section
        "butter5_padded": signal.butter(5, 0.2, output="sos"),        # 3 sections padded to 4
        "fast_real": real_pair(0.3, -0.2),                            # every scan level skipped
        "near_double": real_pair(0.9, 0.8999),                        # real Schur basis
        "smoother_f32": smoother_f32(0.95),
        "near_double_mid4": np.vstack([b8[:1], real_pair(0.5, 0.49999), b8[1:2]]),
        "near_double_mid6": np.vstack([b8[:2], real_pair(0.95, 0.95 - 1e-5), b8[2:4]]),
    }


# name -> (padded section count, unit-numerator form, flags of every padded section, a first-order section present)
# flags: bits 0..3 = in-row scan level 2^i skipped, bit 4 = SA_IIR_SKIP_ROWSCAN (csrc/sa_common.hpp)
CASCADE_VARIANTS = {
    "butter12": (6, 1, (31, 31, 31, 30, 30, 24), False),
    "rtl_default": (6, 0, (24, 24, 24, 24, 24, 24), False),
    "long_memory": (2, 1, (0, 0), False),
    "butter3_first_order": (2, 0, (31, 31), True),
    "butter5_padded": (4, 0, (31, 31, 28, 31), True),
    "fast_real": (2, 0, (31, 31), False),
    "near_double": (2, 0, (24, 31), False),
    "smoother_f32": (2, 0, (16, 31), False),
    "near_double_mid4": (4, 0, (30, 31, 30, 31), False),
    "near_double_mid6": (6, 0, (30, 30, 16, 28, 24, 31), False),
}


def plan_header(plan):
    """(nsec, unit, wingen, [flags of the six section slots]) of an exported float plan."""
    nsec = int(plan[:1].view(np.int32)[0])
    unit = int(plan[1:2].view(np.int32)[0])
    wingen = int(plan[3:4].view(np.int32)[0])
    flags = [int(plan[4 + 48 * s + 5:4 + 48 * s + 6].view(np.int32)[0]) for s in range(6)]
    return nsec, unit, wingen, flags
