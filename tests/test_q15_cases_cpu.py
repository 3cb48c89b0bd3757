"""CPU: tests/q15_cases.py keeps what it promises the GPU tests of the integer chain -- every cascade in its table passes
signal, fixture G4's wide cascade (which the table replaced) passes none, and the table and the files agree on the names."""
import importlib

import numpy as np

from conftest import N, load_golden
from q15_cases import GUI_UPLOAD, SETUPS, chain_args, uniform, wide_sections

# file -> the setups it parametrizes over or configures by name
USERS = {
    "test_gpu_q15_trace": lambda m: m.FORMS,
    "test_gpu_q15_trace_avg": lambda m: m.FORMS,
    "test_gpu_q15_spectra": lambda m: m.FORMS,
    "test_gpu_q15_hop": lambda m: m.MODES,
    "test_gpu_q15_p12": lambda m: m.MODES,
    "test_gpu_q15_outputs": lambda m: [row[0] for row in m.FORMS.values()],
    "test_gpu_isolation": lambda m: m.Q15_CASES,
}


def _live(t):
    """the smallest fraction of non-zero samples among the frames of a time series"""
    return float((t != 0).mean(axis=1).min())


def test_every_cascade_of_the_table_passes_signal(oracle):
    """For every setup with a cascade (any filter byte but 0xB1; 0xA2 with at least one section), and for every prefix
    wide_sections()[:n], n = 1 .. 6, in both window modes: two uniform random frames at 12-bit scale and two at full scale
    (seed 0 for a custom ROM, seed 0 for the frames); in each frame more than half of the samples of the integer model's
    time series are non-zero.  Measured, the lower frame of each pair, at 12-bit scale / at full scale: the GUI upload 0.831 /
    0.836 under the RTL window, 0.828 / 0.837 in the 16-bit Hann reading, 0.737 / 0.845 under a random ROM (the lowest of
    all); custom_nob1 0.994 / 0.999; the fixed ALPHA / BETA set (mode 0x00, and uploaded as 0xA1-zero-b1) 0.994 / 1.000, under
    a random ROM in the Hann reading 0.997 / 1.000; the prefixes of wide_sections() 0.996 .. 0.998 / 1.000 in window mode 0,
    0.969 .. 0.971 / 0.991 .. 0.992 in window mode 1, 0.999 / 1.000 under a random ROM."""
    cases = {name: chain_args(name, np.random.default_rng(0)) for name, s in SETUPS.items()
             if s.cmd != 0xB1 and (s.cmd != 0xA2 or s.nsec)}
    assert len(cases) >= 15, sorted(cases)
    cases.update({f"wide_sections()[:{n}] window mode {wm}": (None, wm, 0xA2, None, wide_sections()[:n])
                  for n in range(1, 7) for wm in (0, 1)})
    for name, args in cases.items():
        rng = np.random.default_rng(0)
        for full in (False, True):
            _, t = oracle.chain_q15(uniform(rng, (2, N), full), *args, want_time=True)
            print(f"FIGURE live samples {name} {'full scale' if full else '12-bit'}: {_live(t):.3f}")
            assert _live(t) > 0.5, (name, full, _live(t))


def test_fixture_g4_wide_cascade_passes_nothing(oracle):
    """Why no frame comparison takes its sections from fixture G4: designer.quantize_sos_q14 keeps the designed gain in section
    0's numerator, where it rounds to zero -- [0, 0, 0, 16384, -16749, 4319] -- so every prefix that contains section 0 gives an
    all-zero time series and an all-zero IQ frame, whatever the input.  (tests/test_host_logic.py::test_q14_quantiser holds the
    quantised design of fixture G2 equal to G4's sections; they are taken from there.)  Without section 0 signal passes."""
    from fpga_real_time_fft_analyzer_amd import designer
    sos = designer.quantize_sos_q14(load_golden("g2_config1.npz")["sos"])
    assert sos.shape == (6, 6) and sos[0].tolist() == [0, 0, 0, 16384, -16749, 4319]
    assert np.array_equal(load_golden("g4_q15_frames.npz")["c_gui"], GUI_UPLOAD)       # G4's upload is the table's
    rng = np.random.default_rng(0)
    x = np.concatenate([uniform(rng, (2, N)), uniform(rng, (2, N), True)])
    for n in range(1, 7):
        for wm in (0, 1):
            iq, t = oracle.chain_q15(x, None, wm, 0xA2, None, sos[:n], want_time=True)
            assert not t.any() and not iq.any(), (n, wm)
    _, t = oracle.chain_q15(x, None, 0, 0xA2, None, sos[1:3], want_time=True)
    assert t.any(axis=1).all()


def test_no_missing_and_no_dead_setup():
    """Every name a test file parametrizes over is in the table, and the table has no setup that no file uses."""
    used = set()
    for module, names in USERS.items():
        names = set(names(importlib.import_module(module)))
        assert names and names <= set(SETUPS), (module, sorted(names - set(SETUPS)))
        used |= names
    assert used == set(SETUPS), sorted(set(SETUPS) - used)
