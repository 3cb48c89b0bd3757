"""Shared by the GPU tests of the integer chain (a plain module, like structured_cases.py and gpu_support.py: no fixtures,
importable without a GPU): the coefficient uploads, the wide cascade, the table of chain setups the test files
parametrize over and the function that puts a handle into one, the sample makers, the dispatcher over the kinds of
call and the by-bits compare of a record tensor.  tests/test_q15_cases_cpu.py holds the table to what it promises: every
cascade in it passes signal, every name a file uses is in it, and it has no setup that no file uses."""
import collections
import functools

import numpy as np

from conftest import N
from q15_mirrors import bits

# ---------------------------------------------------------------------------------------------- coefficient uploads
# 12 bytes in wire order b0,b1,b2,a0,a1,a2 per set.  GUI_UPLOAD: the defaults of gui.py:159-179, 1186-1192; B1 != 0, the long
# (nine-instruction) step.  ZERO_B1_C12: the fixed ALPHA / BETA set of imp/filter_pkg.vhd:54-68, what mode 0x00 runs; B1 = 0 in
# both sets, the short step.  C12_NOB1: the GUI's feedback taps with B1 = 0 in both sets.
GUI_UPLOAD = np.array([0, 1, 0, 64, -67, 19, 64, 127, 64, 64, -85, 40], np.int8)
ZERO_B1_C12 = np.array([-14, 0, 14, 107, 21, 127, -15, 0, 15, 107, -21, 127], np.int8)
C12_NOB1 = np.array([32, 0, -32, 64, -67, 19, 64, 0, 64, 64, -85, 40], np.int8)
for _a in (GUI_UPLOAD, ZERO_B1_C12, C12_NOB1):
    _a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def wide_sections():
    """Six Q2.14 sections that let the test frames through: second-order Butterworth low-passes of unity DC gain,
    cut-offs 0.35 .. 0.85 of Nyquist.  (The golden file's cascade carries its whole gain in the first section, whose
    numerator rounds to zero in Q2.14: every output is zero, and a comparison of zeros shows nothing.)"""
    from scipy import signal
    sos = np.concatenate([signal.butter(2, wc, output="sos") for wc in (0.35, 0.45, 0.55, 0.65, 0.75, 0.85)])
    q = np.rint(sos * 16384.0)
    assert q.shape == (6, 6) and np.abs(q).max() <= 32767 and (q[:, 0] > 0).all()
    q = q.astype(np.int16)
    q.setflags(write=False)
    return q


# --------------------------------------------------------------------------------------------------- chain setups
# cmd: the filter byte.  c12: the 12-byte upload, or None.  nsec: None leaves the handle's Q2.14 sections alone, 0..6 loads
# that many of wide_sections() (0 is the wire).  win_mode: 0 the RTL window, 1 the unsigned-Hann reading of the ROM.
# custom_rom: a random window ROM, drawn by configure().
Setup = collections.namedtuple("Setup", "cmd c12 nsec win_mode custom_rom")

SETUPS = {
    "b1_rtl": Setup(0xB1, None, None, 0, False),
    "b1_hann_u16": Setup(0xB1, None, None, 1, False),
    "b1_rom_rtl": Setup(0xB1, None, None, 0, True),
    "b1_rom_hann_u16": Setup(0xB1, None, None, 1, True),
    "default": Setup(0x00, None, None, 0, False),
    "default_rom_hann_u16": Setup(0x00, None, None, 1, True),
    "gui_upload": Setup(0xA1, GUI_UPLOAD, None, 0, False),
    "gui_upload_rom": Setup(0xA1, GUI_UPLOAD, None, 0, True),
    "gui_upload_hann_u16": Setup(0xA1, GUI_UPLOAD, None, 1, False),
    "wide0": Setup(0xA2, None, 0, 0, False),
    "wide1": Setup(0xA2, None, 1, 0, False),
    "wide2": Setup(0xA2, None, 2, 0, False),
    "wide2_hann_u16": Setup(0xA2, None, 2, 1, False),
    "wide3": Setup(0xA2, None, 3, 0, False),
    "wide3_rom": Setup(0xA2, None, 3, 0, True),
    "wide4": Setup(0xA2, None, 4, 0, False),
    "wide5_rom_hann_u16": Setup(0xA2, None, 5, 1, True),
    "wide6": Setup(0xA2, None, 6, 0, False),
    "wide6_hann_u16": Setup(0xA2, None, 6, 1, False),
    "0xA1-zero-b1": Setup(0xA1, ZERO_B1_C12, None, 0, False),
    "custom_nob1": Setup(0xA1, C12_NOB1, None, 0, False),
}
# the same setups as tests/test_gpu_q15_hop.py, test_gpu_q15_p12.py and test_gpu_isolation.py spell them in their test ids
# (the latter two set the window mode themselves)
SETUPS.update({alias: SETUPS[name] for alias, name in (
    ("b1_rom", "b1_rom_rtl"), ("0xB1", "b1_rtl"), ("0x00", "default"), ("0xA1-b1", "gui_upload"), ("0xA2-six", "wide6"),
    ("0xA2-none", "wide0"), ("bypass", "b1_rtl"), ("custom_b1", "gui_upload"))})
SETUP_OF_MODE = {0xB1: "b1_rtl", 0x00: "default", 0xA2: "wide6"}          # for the tests that go by the filter byte alone


def chain_args(setup, rng=None):
    """oracle.chain_q15's arguments after x for SETUPS[setup]: (rom, win_mode, cmd, c12, sos_q14).  A custom ROM is drawn
    from `rng`, which only a setup with one needs."""
    cmd, c12, nsec, wm, custom_rom = SETUPS[setup]
    rom = rng.integers(-32768, 32768, size=N).astype(np.int16) if custom_rom else None
    return rom, wm, cmd, c12, None if nsec is None else wide_sections()[:nsec]


def configure(ch, setup, rng=None):
    """Put the handle into SETUPS[setup]; returns chain_args(setup, rng).  The ROM is drawn before anything the caller
    draws from `rng` afterwards."""
    rom, wm, cmd, c12, sos14 = args = chain_args(setup, rng)
    if rom is not None:
        ch.set_window_q15(rom)
    ch.set_window_mode_q15(wm)
    if c12 is not None:
        ch.load_coeffs_q7(c12)
    if sos14 is not None:
        ch.load_sos_q14(sos14)
    ch.set_filter_mode(cmd)
    return args


# ------------------------------------------------------------------------------------------------------- samples
def sample_range(full_scale):
    """(lo, hi) of a uniform draw: the whole int16 range, or 12 bits"""
    return (-32768, 32768) if full_scale else (-2048, 2048)


def uniform(rng, shape, full_scale=False):
    """uniform random int16 samples from `rng`, 12-bit or full-scale"""
    return rng.integers(*sample_range(full_scale), size=shape).astype(np.int16)


def extreme_frames(zero_frame=False):
    """Constant +32767, constant -32768, alternating extremes, a lone -32768 impulse; with `zero_frame` an all-zero frame
    behind them."""
    x = np.zeros((4 + bool(zero_frame), N), np.int16)
    x[0] = 32767
    x[1] = -32768
    x[2, ::2] = 32767
    x[2, 1::2] = -32768
    x[3, 0] = -32768
    return x


# --------------------------------------------------------------------------------------------------------- calls
def call(ch, kind, x, hop=None, out=None):
    """One call of kind `kind` on x [at hop] [into out]: "filter" (the time series; frames only), an out_kind of
    process_q15, or a number: the display trace with buckets of that many bins."""
    if kind == "filter":
        return ch.filter_q15(x, out)
    if isinstance(kind, int):
        return ch.traces_q15(x, bucket=kind, out=out, hop=hop)
    return ch.process_q15(x, out=out, out_kind=kind, hop=hop)


def handle_iq(ch, xd):
    """the reference frames of the grouped kinds: the handle's own IQ call on the same input, on the host"""
    return ch.process_q15(xd, out_kind="iq").cpu().numpy()


def records_equal(rec, peak, power, shape, tag):
    """a [..., 2] float32 {peak_mag, power} record tensor of shape `shape` against numpy's `peak` and `power`, by bits;
    `tag` is the tuple a failure begins with"""
    assert tuple(rec.shape) == shape and str(rec.dtype) == "torch.float32", tag + (rec.shape, rec.dtype)
    r = rec.cpu().numpy()
    for i, (name, want) in enumerate((("peak", peak), ("power", power))):
        bad = np.nonzero(bits(r[..., i]) != bits(want))
        assert bad[0].size == 0, tag + (name, bad[0][:5], bad[1][:5], r[..., i][bad][:5], want[bad][:5])
