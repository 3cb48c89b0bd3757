"""GPU: the fused float chain at the smallest batches -- B = 1 (a lone workgroup), 3 and 5 (more workgroups than one, placed
on CUs that hold nothing else) -- in every input form, every spectrum kind and the three filter modes, against the float64
oracle and form against form.

What these batches can catch and the large ones of the other modules hide: a workgroup that starts on a CU no earlier
workgroup has prepared.  The kernels keep two tables in LDS that they copy there themselves, once per workgroup -- the
per-lane scan matrices of the cascade and the pass-B twiddles W_256^(k b) -- and a read that ran ahead of the copy, or a
copy that missed part of a table, shows in the first frame a CU sees.  (tests/test_gpu_isolation.py poisons the LDS in
front of such frames; here the results are held to the oracle.)

Bounds: TOL = 1e-5 of tests/test_gpu_f32.py, max-norm per frame, on the magnitudes and on the complex spectrum.  For the
marker record: the peak within TOL of the frame's reference peak P, and the band power within 3e-5 of the reference power
S, the bound of tests/test_gpu_marker.py::test_marker_against_float64_oracle (a sum of squares of values each within
TOL * P is not within TOL * S); the peak is also the maximum of the mag_full row bit for bit, as that module asserts.
Between forms: the int16 call on samples s and the float32 call on float32(s) * scale agree bit for bit (scale = 2^-11 is
exact), and the packed call agrees with the int16 call on the same 12-bit samples.
First MI355X run, worst over the nine cases: magnitudes 1.2e-6, spectrum 1.2e-6, peak 3.9e-7 P, power 4.1e-7 S; the forms
bit-identical in every kind.  The module also passes on the commit before the tables moved (3 s for the nine cases)."""
import numpy as np
import pytest

from conftest import N, load_golden, rel_maxnorm
from gpu_support import ch, to_device, torch_mod  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
TOL = 1e-5
POWER_TOL = 3e-5
SCALE = 1.0 / 2048
BATCHES = (1, 3, 5)
MODES = (0xA1, 0xB1, 0x00)
KINDS = ("mag_full", "mag_half", "spec_half", "marker")
FORMS = ("float32", "int16", "uint8")          # uint8: the int16 samples packed to 12 bits (ingest.pack12)

# filter 0x00 on the float path: the RTL's default taps as reals (tests/test_gpu_f32.py)
_A = [14 / 128, 0, -14 / 128, 1, 21 / 128, 107 / 128]
_B = [15 / 128, 0, -15 / 128, 1, -21 / 128, 107 / 128]
RTL_SOS = np.array([_A, _B, _A, _B, _A, _B])


def _samples(B):
    """12-bit samples: a tone per frame plus noise, the last frame an impulse in mid-frame (a flat spectrum)."""
    rng = np.random.default_rng(1000 + B)
    n = np.arange(N)
    x = 0.8 * np.sin(2 * np.pi * rng.uniform(0.01, 0.45, (B, 1)) * n) + 0.05 * rng.standard_normal((B, N))
    if B > 1:
        x[-1] = 0.0
        x[-1, N // 2 + 3] = 0.9
    return np.rint(x * 2048).clip(-2048, 2047).astype(np.int16)


_REF = {}


def _reference(oracle, B, mode):
    """(samples, X [B, 8193], mag [B, 16384]) in float64, computed once per (B, mode) and left unchanged."""
    if (B, mode) not in _REF:
        s = _samples(B)
        x = s.astype(np.float32) * np.float32(SCALE)
        sos = {0xA1: load_golden("g2_config1.npz")["sos"], 0xB1: None, 0x00: RTL_SOS}[mode]
        _, X, mag = oracle.chain_fp(x, sos)
        for a in (s, X, mag):
            a.setflags(write=False)
        _REF[(B, mode)] = (s, X, mag)
    return _REF[(B, mode)]


def _inputs(torch_mod, s):
    from fpga_real_time_fft_analyzer_amd.ingest import pack12
    return {"float32": (to_device(torch_mod, s.astype(np.float32) * np.float32(SCALE)), {}),
            "int16": (to_device(torch_mod, s), {"scale": SCALE}),
            "uint8": (to_device(torch_mod, pack12(s)), {"scale": SCALE})}


@pytest.mark.parametrize("mode", MODES, ids=lambda m: f"0x{m:02X}")
@pytest.mark.parametrize("B", BATCHES)
def test_small_batches_every_form_and_kind(ch, torch_mod, oracle, B, mode):
    s, X, mag = _reference(oracle, B, mode)
    if mode == 0xA1:
        ch.load_sos(load_golden("g2_config1.npz")["sos"])
    ch.set_filter_mode(mode)
    ch.set_marker_range(0, N)
    P, S = mag.max(axis=1), (mag ** 2).sum(axis=1)
    assert (P > 0).all()
    got = {}
    for form, (xd, kw) in _inputs(torch_mod, s).items():
        for kind in KINDS:
            got[form, kind] = ch.process_f32(xd, out_kind=kind, **kw).cpu().numpy()
    figures = []
    for form in FORMS:
        full, half, spec, rec = (got[form, k] for k in KINDS)
        e_full = rel_maxnorm(full, mag)
        e_half = rel_maxnorm(half, mag[:, :N // 2 + 1])
        e_spec = float((np.abs(spec - X).max(axis=1) / np.abs(X).max(axis=1)).max())
        pm, pb, bp = rec[:, 0].view(np.float32), rec[:, 1], rec[:, 2].view(np.float32)
        e_peak = float((np.abs(pm - P) / P).max())
        e_pow = float((np.abs(bp - S) / S).max())
        figures.append(f"{form}: full {e_full:.2e} half {e_half:.2e} spec {e_spec:.2e} peak {e_peak:.2e} power {e_pow:.2e}")
        print(f"FIGURE small batch B={B} mode 0x{mode:02X} {figures[-1]}")
        assert full.shape == (B, N) and half.shape == (B, N // 2 + 1) and spec.shape == (B, N // 2 + 1) and rec.shape == (B, 4)
        assert e_full <= TOL and e_half <= TOL and e_spec <= TOL, figures[-1]
        assert e_peak <= TOL and e_pow <= POWER_TOL, figures[-1]
        # the mirrored halves of the magnitude row, the half row, and the marker's peak: one set of values
        assert np.array_equal(full[:, N // 2 + 1:], full[:, 1:N // 2][:, ::-1])
        assert np.array_equal(half, full[:, :N // 2 + 1])
        assert np.array_equal(pm.view(np.uint32), full.max(axis=1).view(np.uint32))
        assert np.array_equal(pb, full.argmax(axis=1))
    for kind in KINDS:
        for form in ("int16", "uint8"):
            assert np.array_equal(got[form, kind].view(np.uint8), got["float32", kind].view(np.uint8)), (form, kind)
