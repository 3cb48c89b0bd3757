"""GPU: the addresses of the fused float chain -- where the stage-in puts a sample, where the FFT's natural-order image and the
split step look for a bin, and what the cascade's scan reads from the neighbouring rows -- at the smallest batches at which
one can be wrong: B = 1 (the first workgroup alone), 3 and 5.

1. Stage-in permutation: position-coded frames through the time-series output with a unit window and no filtering (the
   cascade bypassed, and a cascade of identity sections, which is exact).  Every sample carries its own position, so a
   wrong row, chunk or swizzle column shows as a wrong value: the output equals the input bit for bit, in the three input
   forms.  float32 frames are x[n] = 1 + n / 16384 + f (exact in float32); int16 frames s[n] = n - 8192 + f; packed frames
   carry 12 bits, s[n] = (n + 37 f) mod 4095 - 2047, whose period is no multiple of a row (64), a slab (512) or a wave's
   share of the frame (4096).
2. Exchange and split positions: a unit cosine exactly on bin k per frame, for the bins next to every seam of the split
   step (the group of four, the image rows of 512 bins, the two rounds at 2048 and 6144, the side slots, thread 0 and
   thread 255).  The peak sits on k, the mirrored halves agree bit for bit, and the row agrees with numpy.fft.fft within
   TOL = 1e-5 of tests/test_gpu_f32.py (the bound of the full-magnitude tests; tests/gpu_support.py holds none); the
   half-spectrum kinds and the marker against the same reference (marker power: POWER_TOL of
   tests/test_gpu_f32_small_batches.py).  Bypassed (B = 16 takes the one-round kernels) and behind the identity cascade
   (the two-round kernels, whose image accesses are written out).
3. Scan constants: unit impulses next to the row seam (n = 1023, 1024), the wave seam (4095, 4096) and at the end of the
   frame (16383) through config 1's cascade, time-series output against scipy.signal.sosfilt in float64, within the bound
   tests/test_gpu_f32.py::test_config1_tone_full_chain applies to config 1's time series, max(TOL, 2 x the error of a
   sequential float32 evaluation); once more with a two-section design (the two-section kernels).
"""
import numpy as np
import pytest

from conftest import N, load_golden, rel_maxnorm
from gpu_support import ch, table_window, to_device, torch_mod  # noqa: F401 (fixtures)
from test_gpu_f32 import TOL
from test_gpu_f32_small_batches import POWER_TOL

pytestmark = pytest.mark.gpu
SCALE = 1.0 / 2048
IDENTITY = [1.0, 0.0, 0.0, 1.0, 0.0, 0.0]
SEAM_BINS = (1, 3, 4, 5, 1023, 1024, 2044, 2047, 2048, 2049, 4095, 4096, 6143, 6144, 8191, 8192)
IMPULSES = (1023, 1024, 4095, 4096, 16383)


def _identity(ch, nsec):
    ch.load_sos(np.array([IDENTITY] * nsec))
    ch.set_filter_mode(0xA1)


# ---------------------------------------------------------------------------------------------- 1. stage-in permutation
@pytest.mark.parametrize("B", (1, 3, 5))
def test_stage_in_puts_every_sample_in_its_place(ch, torch_mod, B):
    from fpga_real_time_fft_analyzer_amd.ingest import pack12
    n, f = np.arange(N)[None, :], np.arange(B)[:, None]
    x32 = (1.0 + n / 16384.0 + f).astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), 1.0 + n / 16384.0 + f)                 # the code is exact
    s16 = (n - 8192 + f).astype(np.int16)
    s12 = ((n + 37 * f) % 4095 - 2047).astype(np.int16)
    forms = {"float32": (to_device(torch_mod, x32), {}, x32),
             "int16": (to_device(torch_mod, s16), {"scale": SCALE}, s16.astype(np.float32) * np.float32(SCALE)),
             "uint8": (to_device(torch_mod, pack12(s12)), {"scale": SCALE}, s12.astype(np.float32) * np.float32(SCALE))}
    ch.set_window_f32(np.ones(N, np.float32))
    for label, setup in (("bypass", lambda: ch.set_filter_mode(0xB1)), ("identity x 6", lambda: _identity(ch, 5)),
                         ("identity x 2", lambda: _identity(ch, 1))):
        setup()
        for form, (xd, kw, want) in forms.items():
            got = ch.process_f32(xd, out_kind="time", **kw).cpu().numpy()
            wrong = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
            print(f"FIGURE stage-in B={B} {label} {form}: {wrong.size} samples out of place")
            assert wrong.size == 0, (label, form, "first at frame, sample", divmod(int(wrong[0]), N))


# ------------------------------------------------------------------------------------- 2. exchange and split positions
_TONES = {}


def _tones():
    """(x [16, N] float32, X = fft of it in float64 [16, N] complex), computed once and left unchanged."""
    if not _TONES:
        n = np.arange(N)
        x = np.cos(2 * np.pi * np.array(SEAM_BINS)[:, None] * n[None, :] / N).astype(np.float32)
        X = np.fft.fft(x.astype(np.float64), axis=-1)
        for a in (x, X):
            a.setflags(write=False)
        _TONES["x"], _TONES["X"] = x, X
    return _TONES["x"], _TONES["X"]


@pytest.mark.parametrize("cascade", ("bypass", "identity x 6"))
def test_tones_on_the_seams_of_the_split_step(ch, torch_mod, cascade):
    x, X = _tones()
    H = N // 2 + 1
    mag = np.abs(X)
    ch.set_window_f32(np.ones(N, np.float32))
    if cascade == "bypass":
        ch.set_filter_mode(0xB1)
    else:
        _identity(ch, 5)
    ch.set_marker_range(0, N)
    xd = to_device(torch_mod, x)
    full = ch.process_f32(xd, out_kind="mag_full").cpu().numpy()
    half = ch.process_f32(xd, out_kind="mag_half").cpu().numpy()
    spec = ch.process_f32(xd, out_kind="spec_half").cpu().numpy()
    rec = ch.process_f32(xd, out_kind="marker").cpu().numpy()
    assert full.shape == (16, N) and half.shape == (16, H) and spec.shape == (16, H) and rec.shape == (16, 4)
    P, S = mag.max(axis=1), (mag ** 2).sum(axis=1)
    for i, k in enumerate(SEAM_BINS):
        e_full = rel_maxnorm(full[i:i + 1], mag[i:i + 1])
        e_half = rel_maxnorm(half[i:i + 1], mag[i:i + 1, :H])
        e_spec = float(np.abs(spec[i] - X[i, :H]).max() / np.abs(X[i, :H]).max())
        pm, pb, bp = rec[i:i + 1, 0].view(np.float32)[0], int(rec[i, 1]), rec[i:i + 1, 2].view(np.float32)[0]
        e_peak, e_pow = abs(pm - P[i]) / P[i], abs(bp - S[i]) / S[i]
        print(f"FIGURE split {cascade} bin {k}: full {e_full:.2e} half {e_half:.2e} spec {e_spec:.2e} "
              f"peak {e_peak:.2e} power {e_pow:.2e}")
        assert int(full[i].argmax()) == k and int(half[i].argmax()) == k and pb == k, (k, int(full[i].argmax()), pb)
        assert np.array_equal(full[i, 1:N // 2].view(np.uint32), full[i, N // 2 + 1:][::-1].view(np.uint32)), k
        assert e_full <= TOL and e_half <= TOL and e_spec <= TOL, (k, e_full, e_half, e_spec)
        assert e_peak <= TOL and e_pow <= POWER_TOL, (k, e_peak, e_pow)
    assert np.array_equal(half.view(np.uint32), full[:, :H].view(np.uint32))


# -------------------------------------------------------------------------------------------------- 3. scan constants
def _impulse_frames(n0):
    """B = 3: the impulse, its negative, and all five impulses in one frame."""
    x = np.zeros((3, N), np.float32)
    x[0, n0] = 1.0
    x[1, n0] = -1.0
    x[2, list(IMPULSES)] = 1.0
    return x


@pytest.mark.parametrize("nsec", (6, 2))
def test_impulses_on_the_seams_of_the_scan(ch, torch_mod, oracle, nsec):
    from scipy.signal import sosfilt
    sos = np.asarray(load_golden("g2_config1.npz")["sos"], np.float64)[:nsec]
    w = table_window()
    ch.set_window_f32(w)
    ch.load_sos(sos)
    ch.set_filter_mode(0xA1)
    for n0 in IMPULSES:
        x = _impulse_frames(n0)
        xw = x.astype(np.float64) * w.astype(np.float64)
        ref = sosfilt(sos, xw, axis=-1)
        seq = max(rel_maxnorm(oracle.sosfilt_f32_c(sos, xw[i].astype(np.float32))[None, :], ref[i:i + 1]) for i in range(3))
        got = ch.process_f32(to_device(torch_mod, x), out_kind="time").cpu().numpy()
        err = rel_maxnorm(got, ref)
        print(f"FIGURE scan {nsec} sections impulse at {n0}: {err:.2e} (sequential float32 {seq:.2e})")
        assert err <= max(TOL, 2 * seq), (nsec, n0, err, seq)
