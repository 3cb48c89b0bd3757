"""Shared by tests/test_window_cases_cpu.py (CPU) and tests/test_gpu_f32_window.py (GPU), a plain module like
structured_cases.py: the named float windows, the verdict fit_cosine_window (csrc/sa_tables.cpp) must give on each, the
bound on a generated window, the four test frames, the table of kernel forms the GPU tests run them through, and the
gates, as functions of plain arrays so that the CPU tests can apply them to a numpy model of a defective kernel.

Why these windows.  Every other float window of the suite (Hann, Hamming, Blackman, ones, gpu_support.table_window) is
smooth and symmetric: a kernel that reads w[n^1], w[n+4], the other half-chunk or w[N-1-n] moves such a window by less
than any gate notices.  `coded` is position-coded -- 0.25 + 0.75 perm[n] / N with a seeded permutation, 16384 distinct
float32 values at least 4.5e-5 apart, not symmetric -- so an exchange of any two samples in any of the device layouts
moves a sample by at least 4.5e-5 of the peak, against gates of 2^-23 = 1.2e-7.  `coded_zeros` adds exact zeros and two
negative entries on the chunk, thread and half-frame seams.  The five accepted windows take the generator of the IIR
kernels (below); `hann_in` / `hann_out` sit on either side of the fit's threshold.

The generated window and its bound A(w).  When fit_cosine_window accepts a table as a0 - a1 cos(theta n), theta =
2 pi / (N-1), within 1.5e-7 of its peak, the IIR spectrum kernels of the float32 precision do not read it; with
n = 64 t + 32 h + j, S = 0.5 * (folded cascade gain) they evaluate (build_plan in csrc/iir_plan.cpp, stage_in_chunks in
csrc/chain_f32.hpp)
    W[n] = fmaf(Q, s_j, fmaf(P, c_j, G0)),   G0 = f32(S a0),  (P, Q) = f32(S a1 (-cos, sin)(theta (64 t + 32 h))),
                                             (c_j, s_j) = f32((cos, sin)(theta j)),
and the applied window is W[n] / S.  Against the loaded table w, as a fraction of the table's peak,
    |W[n] / S - w[n]| / peak  <=  A(w) = 1.5e-7 + 5 * 2^-24 * (|a0| + |a1|) / peak :
  - 1.5e-7: the table's distance from the fitted formula, the fit's own acceptance threshold;
  - the formula in exact arithmetic is S a0 + P c + Q s, where P c + Q s = -S a1 cos(phi + theta j), phi = theta (64 t +
    32 h).  Five float32 roundings separate W[n] from it, each a relative 2^-24 at most:
      of G0:             2^-24 S |a0|;
      of the pair P, Q:  2^-24 (|P c| + |Q s|) = 2^-24 S |a1| (|cos phi cos theta j| + |sin phi sin theta j|)
                         = 2^-24 S |a1| max |cos(phi -+ theta j)| <= 2^-24 S |a1|;
      of the pair c, s:  the same sum, <= 2^-24 S |a1|;
      of the inner FMA:  2^-24 |P c + G0| <= 2^-24 S (|a0| + |a1|);
      of the outer FMA:  2^-24 |W[n]|     <= 2^-24 S (|a0| + |a1|).
    Each is at most 2^-24 of a term no larger than S (|a0| + |a1|); their sum is 2^-24 S (3 |a0| + 4 |a1|), which with
    the products of two roundings (2^-48) and libm's double cos / sin stays under 5 * 2^-24 S (|a0| + |a1|).
For Hann (a0 = a1 = 0.5, peak 1) A = 4.5e-7.  A numpy float32 emulation of the formula gives at worst 2.0e-7 on the
accepted windows below, at gain 1 and at the folded gain of butter(12, 0.2) (1.2e-7).  The bound is derived, not fitted
to an output.  It is ABSOLUTE (a fraction of the peak): at n = 1 Hann is 3.7e-8, below the generator's resolution
(include/specan.h, sa_set_window_f32, says so).

What runs the generator.  The fused spectrum kernels (chain_f32_kernel, chain_marker_kernel) with a cascade.  The
'time' output kind (time_f32_kernel) always reads the plan's table copy win_t (0.5 * w * gain, transposed), and so do
bypass mode and the float64-state precision.  The generator's tables are therefore held per sample on the host
(test_window_cases_cpu.py) and its use by the kernels through the spectrum (gate T3); gate T2 on 'time' holds the plan's
table copy of an accepted window to the same absolute bound."""
import functools
import re
from typing import NamedTuple, Optional

import numpy as np
from scipy import signal

import kernel_inventory as ki
import structured_cases as sc

N = 16384
H = N // 2 + 1
THETA = 2.0 * np.pi / (N - 1)
FIT_THRESHOLD = 1.5e-7                      # csrc/sa_tables.cpp, fit_cosine_window
ONE_ROUND_MAX = 512                         # csrc/chain_f32.hpp, kOneRoundMax: float32 frames of the bypassed chain

# name -> the verdict of the fit: True = accepted (the IIR spectrum kernels generate it), False = refused (table)
VERDICTS = {"hann_default": True, "hann_table": True, "hamming": True, "cos_neg": True, "hann_in": True,
            "hann_out": False, "coded": False, "coded_zeros": False}
ACCEPTED = tuple(k for k, v in VERDICTS.items() if v)
REFUSED = tuple(k for k, v in VERDICTS.items() if not v)
SEED_IN, SEED_OUT, SEED_CODED = 11, 12, 13
ZEROS_AT = (0, 1, 31, 32, 63, 64, 8191, 8192, 16383)
NEGATIVE_AT = (100, 8292)


def hann64():
    """The library's default window in double (csrc/sa_tables.cpp, default_window_f64)."""
    return 0.5 * (1.0 - np.cos(THETA * np.arange(N)))


@functools.lru_cache(maxsize=None)
def table(name):
    """The float32 table [N] the window `name` stands for (read-only): what the applied window is compared with."""
    n = np.arange(N)
    if name in ("hann_default", "hann_table"):
        w = hann64()
    elif name == "hamming":
        w = np.hamming(N)
    elif name == "cos_neg":
        w = 0.3 + 0.7 * np.cos(THETA * n)
    elif name in ("hann_in", "hann_out"):
        amp, seed = (1.0e-7, SEED_IN) if name == "hann_in" else (3.0e-7, SEED_OUT)
        w = hann64() + amp * np.random.default_rng(seed).choice([-1.0, 1.0], N)
    elif name in ("coded", "coded_zeros"):
        w = 0.25 + 0.75 * np.random.default_rng(SEED_CODED).permutation(N) / N
        if name == "coded_zeros":
            w[list(ZEROS_AT)] = 0.0
            w[list(NEGATIVE_AT)] = -0.5
    else:
        raise KeyError(name)
    w = w.astype(np.float32)
    w.setflags(write=False)
    return w


def loaded(name):
    """What set_window_f32 is given for `name`: None for the library's own Hann, else the table."""
    return None if name == "hann_default" else table(name)


def fit(w):
    """numpy mirror of fit_cosine_window: (accepted, a0, a1, worst residual as a fraction of the peak)."""
    v = np.asarray(w, np.float64)
    c = -np.cos(THETA * np.arange(N))
    s1, s_c, s_cc, s_w, s_wc = float(N), c.sum(), (c * c).sum(), v.sum(), (v * c).sum()
    peak = np.abs(v).max()
    det = s1 * s_cc - s_c * s_c
    if not (det > 0 and peak > 0 and np.isfinite(peak) and np.isfinite(s_w)):
        return False, 0.0, 0.0, np.inf
    a0, a1 = (s_w * s_cc - s_wc * s_c) / det, (s1 * s_wc - s_c * s_w) / det
    resid = float(np.abs(v - (a0 + a1 * c)).max() / peak)
    return bool(resid <= FIT_THRESHOLD), float(a0), float(a1), resid


def cosine_pair(name):
    """(a0, a1) the plan is built with: (0.5, 0.5) exactly for the library's own Hann, else the fit's."""
    if name == "hann_default":
        return 0.5, 0.5
    ok, a0, a1, _ = fit(table(name))
    assert ok, name
    return a0, a1


def bound_a(a0, a1, peak):
    """A(w) of the module docstring, a fraction of the table's peak."""
    return FIT_THRESHOLD + 5.0 * 2.0 ** -24 * (abs(a0) + abs(a1)) / peak


def bound_of(name, scale=1.0):
    """(A(w), peak) of an accepted window, the table scaled by `scale`; (None, peak) for a refused one."""
    peak = float(np.abs(table(name).astype(np.float64)).max()) * scale
    if not VERDICTS[name]:
        return None, peak
    a0, a1 = cosine_pair(name)
    return bound_a(a0 * scale, a1 * scale, peak), peak


def fmaf(a, b, c):
    """float32 fused multiply-add: the product of two float32 is exact in double, and so is its sum with a float32 up to
    one rounding to 53 bits, 29 bits below the float32 rounding that follows."""
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
            + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def generate(wg0, wgen, wcs):
    """The generator of stage_in_chunks on the host: W[64 t + 32 h + j] = fmaf(Q, s_j, fmaf(P, c_j, G0)), float32 [N],
    from SaIirLaneTab's wg0, wgen [256][4] = (P_0, Q_0, P_1, Q_1) per thread and wcs [32][2] = (c_j, s_j)."""
    pq = np.asarray(wgen, np.float32).reshape(256, 2, 2)
    cs = np.asarray(wcs, np.float32).reshape(32, 2)
    p, q = pq[:, :, 0][:, :, None], pq[:, :, 1][:, :, None]
    return fmaf(q, cs[None, None, :, 1], fmaf(p, cs[None, None, :, 0], np.float32(wg0))).reshape(N)


def transposed(w):
    """win_t of a natural-order table: win_t[(g 256 + t) 4 + e] = w[64 t + 4 g + e]."""
    return np.asarray(w).reshape(256, 16, 4).transpose(1, 0, 2).reshape(N)


# ----------------------------------------------------------------------------------------------------------- the frames
IMPULSE_AT = (0, 31, 32, 63, 64, 1023, 1024, 8191, 8192, 16383)
INT_SCALE = 2.0 ** -10                       # integer forms: sample 1024 is x = 1 exactly (12-bit range: -2048 .. 2047)
FRAME_NAMES = ("ones", "minus_two", "noise", "impulses")


@functools.lru_cache(maxsize=None)
def frames(integer):
    """The four frames, read-only: all ones, all -2, seeded noise, impulses of height 1 at IMPULSE_AT.
    integer False: (float32 [4, N], the same widened).  True: (int16 [4, N] within the 12-bit range, samples * 2^-10)."""
    rng = np.random.default_rng(2025)
    if integer:
        x = np.zeros((4, N), np.int16)
        x[0], x[1], x[2] = 1024, -2048, rng.integers(-2048, 2048, N)
        x[3, list(IMPULSE_AT)] = 1024
        x64 = x.astype(np.float64) * INT_SCALE
    else:
        x = np.zeros((4, N), np.float32)
        x[0], x[1], x[2] = 1.0, -2.0, rng.standard_normal(N)
        x[3, list(IMPULSE_AT)] = 1.0
        x64 = x.astype(np.float64)
    x.setflags(write=False)
    x64.setflags(write=False)
    return x, x64


# ------------------------------------------------------------------------------------------------------------ the gates
def gate_t1(time, xw):
    """Table paths: (worst |time - xw| / |xw| where xw != 0, samples nonzero where xw == 0, samples of the wrong sign).
    Passes when the first is <= 2^-23 and the other two are 0."""
    time, xw = np.asarray(time, np.float64), np.asarray(xw, np.float64)
    nz = xw != 0
    rel = float((np.abs(time - xw)[nz] / np.abs(xw)[nz]).max()) if nz.any() else 0.0
    return rel, int(np.count_nonzero(time[~nz])), int(np.count_nonzero(np.sign(time[nz]) != np.sign(xw[nz])))


def t1_passes(fig):
    return fig[0] <= 2.0 ** -23 and fig[1] == 0 and fig[2] == 0


def gate_t2(time, x, w, a, peak):
    """Generated path, per sample: |time - x w| <= A peak |x| + 2^-24 |x w|.  (worst error / bound over the samples,
    worst |time - x w| / (peak |x|) over the samples with x != 0: the applied window's error as a fraction of the peak).
    Passes when the first is <= 1; a sample with x = 0 must be exactly 0."""
    time, x, w = np.asarray(time, np.float64), np.asarray(x, np.float64), np.asarray(w, np.float64)
    err = np.abs(time - x * w)
    bound = a * peak * np.abs(x) + 2.0 ** -24 * np.abs(x * w)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    nz = x != 0
    return float(ratio.max()), float((err[nz] / (peak * np.abs(x[nz]))).max())


def gate_t3(spec, mag, x, w, a=None, peak=None):
    """Spectrum of the frames x [F, N] under the table w: (spec figure, mag figure, float32-FFT bound, window term) in
    structured_cases.bin_norm against numpy's float64 rfft of x w.  The window term of a generated window is
    A peak sqrt(N) rms(x) / RMS_k |ref_k|, worst frame.  Passes when both figures are <= bound + term."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    xw = x * w
    ref = np.fft.rfft(xw, axis=1)
    b_fft = sc.fft_bound(xw.astype(np.float32), ref)
    term = 0.0
    if a is not None:
        rms_ref = np.sqrt(np.mean(np.abs(ref) ** 2, axis=1))
        term = float((a * peak * np.sqrt((x * x).sum(axis=1)) / rms_ref).max())
    return sc.bin_norm(spec, ref), sc.bin_norm(mag, np.abs(ref)), b_fft, term


def t3_passes(fig):
    return fig[0] <= fig[2] + fig[3] and fig[1] <= fig[2] + fig[3]


# ------------------------------------------------------------------------------------------------------------ the forms
def butter8():
    return signal.butter(8, 0.1, output="sos")


def identity(k):
    return np.tile([1.0, 0, 0, 1.0, 0, 0], (k, 1))


def cascade_sos(name):
    """The SOS a form loads (None: nothing is loaded -- bypass, or mode 0x00 with its fixed taps)."""
    if name is None or name == "rtl_mode00":
        return None
    if name.startswith("identity"):
        return identity(int(name[len("identity"):]))
    return butter8() if name == "butter8" else sc.cascades()[name]


def reference_sos(name):
    """The SOS a float64 reference filters with (None: no cascade, or identity sections: y = x)."""
    if name == "rtl_mode00":
        return sc._rtl6()
    return None if name is None or name.startswith("identity") else cascade_sos(name)


class Form(NamedTuple):
    mode: int                   # filter mode byte
    cascade: Optional[str]      # cascade_sos / reference_sos
    in_form: str                # torch dtype of x: float32, int16, or uint8 = packed 12-bit
    pad: Optional[int]          # batch padded to this many frames
    precision: str
    windows: tuple
    gate: str                   # "T1/T2" (the window's verdict decides), "T1" (always the table) or "T4"
    nsec: int                   # the padded section count the plan must show (0: no plan is launched)
    unit: int


_ALL = tuple(VERDICTS)
_PAIR = ("hamming", "coded")
IN_FORMS = {"f32": "float32", "i16": "int16", "p12": "uint8"}


def _forms():
    f = {"bypass_f32_one_round": Form(0xB1, None, "float32", None, "f32", ("hamming", "coded", "coded_zeros"), "T1", 0, 0),
         "bypass_f32_two_round": Form(0xB1, None, "float32", 513, "f32", ("hamming", "coded", "coded_zeros"), "T1", 0, 0),
         "bypass_i16": Form(0xB1, None, "int16", None, "f32", ("hamming", "coded", "coded_zeros"), "T1", 0, 0),
         "bypass_p12": Form(0xB1, None, "uint8", None, "f32", ("hamming", "coded", "coded_zeros"), "T1", 0, 0)}
    for tag, dt in IN_FORMS.items():
        for k, nsec in ((1, 2), (3, 4), (5, 6)):
            f[f"identity{k}_{tag}"] = Form(0xA1, f"identity{k}", dt, None, "f32", _ALL, "T1/T2", nsec, 0)
    for tag in ("f32", "i16"):
        f[f"mode00_{tag}"] = Form(0x00, "rtl_mode00", IN_FORMS[tag], None, "f32", _PAIR, "T4", 6, 0)
        for casc, nsec in (("butter12", 6), ("butter8", 4), ("long_memory", 2)):
            f[f"unit_{casc}_{tag}"] = Form(0xA1, casc, IN_FORMS[tag], None, "f32", _PAIR, "T4", nsec, 1)
    for tag, dt in IN_FORMS.items():
        f[f"f64_identity2_{tag}"] = Form(0xA1, "identity2", dt, None, "f64", _PAIR, "T1", 2, 0)
        f[f"f64_butter12_{tag}"] = Form(0xA1, "butter12", dt, None, "f64", _PAIR, "T4", 6, 1)
    return f


FORMS = _forms()
KINDS = ("spec_half", "mag_half", "mag_full", "time")


def stage_in(form, window):
    """(InT, nsec, unit, wingen, one_round) of the spectrum kernels of (form, window), as kernel_inventory.float_kernels
    takes them; in f64 precision the bypassed chain behind iir_f64_kernel."""
    fm = FORMS[form]
    batch = fm.pad or 4
    if fm.precision == "f64":
        return ("float32", 0, 0, 0, batch <= ONE_ROUND_MAX)
    one_round = fm.nsec == 0 and fm.in_form == "float32" and batch <= ONE_ROUND_MAX
    return (fm.in_form, fm.nsec, fm.unit, bool(fm.nsec) and VERDICTS[window], one_round)


def launches(form, window):
    """The kernel keys (kernel_inventory) of the four process calls the GPU tests make on (form, window)."""
    fm = FORMS[form]
    keys = []
    for kind in KINDS:
        if fm.precision == "f64":
            variant = (fm.in_form, fm.nsec, fm.unit, False, stage_in(form, window)[4], kind, "f64")
        else:
            variant = (*stage_in(form, window), kind, "f32")
        keys.extend(ki.float_kernels(variant))
    return keys


def stage_in_class(key):
    """(InT, wingen, nsec > 0, one_round) of a chain_f32_kernel key, None for any other kernel."""
    m = re.fullmatch(r"chain_f32_kernel<(\w+), (\d), (true|false), \d, (true|false), (true|false)(, float)?>", key)
    return m and (m.group(1), m.group(4) == "true", int(m.group(2)) > 0, m.group(5) == "true")
