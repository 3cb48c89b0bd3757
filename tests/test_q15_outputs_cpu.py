"""CPU: what the SA_Q15_OUT_* outputs need no GPU for -- the record layout, the constants, the wrapper's out_kind
validation, the C entry point's NULL-handle refusal and the numpy mirror frames.marker_of_frame against fixture G6."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import N, ROOT, load_golden


def _header():
    return open(os.path.join(ROOT, "include", "specan.h")).read()


def test_marker_record_layout():
    """sizeof(sa_marker_q15) == 16 with peak_mag at 0, peak_bin at 4, band_power at 8: the ctypes mirror, and the field
    order and types the header declares."""
    from fpga_real_time_fft_analyzer_amd.abi import MarkerQ15
    assert ctypes.sizeof(MarkerQ15) == 16
    assert (MarkerQ15.peak_mag.offset, MarkerQ15.peak_bin.offset, MarkerQ15.band_power.offset) == (0, 4, 8)
    assert (MarkerQ15.peak_mag.size, MarkerQ15.peak_bin.size, MarkerQ15.band_power.size) == (4, 4, 8)
    body = re.search(r"typedef struct sa_marker_q15 \{(.*?)\} sa_marker_q15;", _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [tuple(f.split()) for f in body.split(";") if f.strip()]
    assert fields == [("float", "peak_mag"), ("int32_t", "peak_bin"), ("uint64_t", "band_power")]
    # a record as the kernel stores it: four little-endian dwords
    raw = np.array([np.float32(507.25).view(np.uint32), 8191, 0x89ABCDEF, 0x1234], np.uint32).tobytes()
    m = MarkerQ15.from_buffer_copy(raw)
    assert (m.peak_mag, m.peak_bin, m.band_power) == (507.25, 8191, (0x1234 << 32) | 0x89ABCDEF)


def test_constants_match_the_header():
    from fpga_real_time_fft_analyzer_amd import abi
    defs = dict(re.findall(r"#define (SA_Q15_OUT_[A-Z]+)\s+(\d+)", _header()))
    assert defs == {"SA_Q15_OUT_IQ": "0", "SA_Q15_OUT_MAG": "1", "SA_Q15_OUT_MARKER": "2"}
    assert (abi.SA_Q15_OUT_IQ, abi.SA_Q15_OUT_MAG, abi.SA_Q15_OUT_MARKER) == (0, 1, 2)
    assert "#define SA_ABI_VERSION 4" in _header()


def test_wrapper_refuses_unknown_kinds_before_touching_the_device(hip_lib_built):
    """out_kind is checked first: no handle, no tensor and no GPU are needed to be told that a name is wrong (the float
    chain's names among them).  The C entry point refuses a NULL handle."""
    from fpga_real_time_fft_analyzer_amd.abi import SA_EINVAL, SpecanError
    from fpga_real_time_fft_analyzer_amd.chain import SpectrumChain
    ch = SpectrumChain.__new__(SpectrumChain)            # no sa_create: there may be no device
    for kind in ("mag_full", "MAG", "", None, 1):
        with pytest.raises(SpecanError) as e:
            ch.process_q15(None, out_kind=kind)
        assert e.value.code == SA_EINVAL
    assert hip_lib_built.sa_process_q15_out(None, None, None, 1, 0, None) == SA_EINVAL


def test_marker_of_frame_on_fixture_g6():
    """The numpy mirror on the reference-pinned frame: g6['mag'] is the reference's own decode_mag_16iq_le of g6['frame']."""
    from fpga_real_time_fft_analyzer_amd import frames
    g6 = load_golden("g6_frame.npz")
    fb = g6["frame"].tobytes()
    mag = g6["mag"]
    assert np.array_equal(frames.decode_mag_16iq_le(fb).view(np.uint32), mag.view(np.uint32))
    iq = np.frombuffer(fb, "<i2").reshape(N, 2)
    for lo, hi in ((0, N), (0, 8193), (100, 2000), (8193, N), (5, 6), (16383, N)):
        pm, pb, bp = frames.marker_of_frame(fb, lo, hi)
        assert isinstance(pm, np.float32) and pm == mag[lo:hi].max() and pb == lo + int(mag[lo:hi].argmax())
        assert mag[pb] == pm and not (mag[lo:pb] == pm).any()                   # the lowest bin attaining it
        assert bp == sum(int(v) * int(v) for v in iq[lo:hi].reshape(-1))         # python integers: no overflow anywhere
    assert frames.marker_of_frame(bytes(65536), 7, 9) == (0.0, 7, 0)
    for lo, hi in ((-1, 5), (5, 5), (0, N + 1)):
        with pytest.raises(ValueError):
            frames.marker_of_frame(fb, lo, hi)
