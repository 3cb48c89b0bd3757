"""CPU: what the display-trace kinds of the integer chain (include/specan.h, SA_Q15_TRACE_KIND) need no GPU for -- the
header's macro, limits and record against abi.py, the kinds' place among the values the other tests refuse, the numpy
mirror frames.trace_of_frame against fixture G6, the wrapper's bucket validation and the shape table."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import N, ROOT, load_golden

WIDTHS = (2, 4, 8, 16, 32, 64)


def _header():
    return open(os.path.join(ROOT, "include", "specan.h")).read()


def test_macro_limits_and_record_match_the_header():
    """The function-like macro, its limits and the 8-byte record: header text against abi.py."""
    from fpga_real_time_fft_analyzer_amd import abi
    h = _header()
    m = re.search(r"#define SA_Q15_TRACE_KIND\((\w+)\)\s+\(0x10 \| \(\1\)\)", h)
    assert m, "SA_Q15_TRACE_KIND must be the function-like macro (0x10 | (log2w))"
    lim = dict(re.findall(r"#define (SA_Q15_TRACE_LOG2W_M(?:IN|AX))\s+(\d+)", h))
    assert lim == {"SA_Q15_TRACE_LOG2W_MIN": "1", "SA_Q15_TRACE_LOG2W_MAX": "6"}
    assert (abi.SA_Q15_TRACE_LOG2W_MIN, abi.SA_Q15_TRACE_LOG2W_MAX) == (1, 6)
    assert [abi.SA_Q15_TRACE_KIND(k) for k in range(1, 7)] == [0x10 | k for k in range(1, 7)] == list(range(17, 23))
    assert "#define SA_ABI_VERSION 4" in h
    body = re.search(r"typedef struct sa_trace_point_q15 \{(.*?)\} sa_trace_point_q15;", h, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [tuple(f.split()) for f in body.split(";") if f.strip()] == [("float", "peak_mag"), ("float", "power")]
    T = abi.TracePointQ15
    assert ctypes.sizeof(T) == 8 and (T.peak_mag.offset, T.power.offset) == (0, 4)
    p = T.from_buffer_copy(np.array([507.25, 3.0e10], np.float32).tobytes())
    assert (p.peak_mag, p.power) == (507.25, float(np.float32(3.0e10)))


def test_trace_kinds_are_disjoint_from_every_refused_and_existing_value():
    """17..22 collide with no kind of either chain and with none of the values the existing tests require to stay
    SA_EINVAL (-1, 3, 7, 99); the neighbours 16 and 23 are not kinds."""
    from fpga_real_time_fft_analyzer_amd import abi, chain
    kinds = {code for code, _, _ in chain.Q15_TRACE_CHAIN.outputs.values()}
    assert kinds == set(range(17, 23))
    assert not kinds & {-1, 3, 7, 99, 16, 23}
    assert not kinds & {code for code, _, _ in chain.Q15_CHAIN.outputs.values()}
    assert not kinds & {code for code, _, _ in chain.FLOAT_CHAIN.outputs.values()}
    # the trace has a table of its own: process_q15 keeps its three kinds
    assert set(chain.Q15_CHAIN.outputs) == {"iq", "mag", "marker"}
    assert sorted(chain.Q15_TRACE_CHAIN.outputs) == list(WIDTHS)
    for dtype, (row, calls) in chain.Q15_TRACE_CHAIN.inputs.items():
        assert {c[0] for c in calls.values()} <= {"sa_process_q15_out", "sa_process_q15_p12"}
        assert all(takes_kind and not takes_scale for _, takes_scale, takes_kind in calls.values())
    assert abi.SA_Q15_TRACE_KIND(4) == chain.Q15_TRACE_CHAIN.output(16)[0]


def test_trace_of_frame_on_fixture_g6():
    """The numpy mirror on the reference-pinned frame, all six widths: the peak is the largest of g6['mag'] (the
    reference's own decode of g6['frame']) in the bucket, the exact sum is python-integer arithmetic, and the power its
    nearest float32, ties to even (checked against an integer rounding made here, not against numpy's conversion)."""
    from fpga_real_time_fft_analyzer_amd import frames
    g6 = load_golden("g6_frame.npz")
    fb = g6["frame"].tobytes()
    mag = g6["mag"]
    iq = np.frombuffer(fb, "<i2").reshape(N, 2)
    ip = [int(r) * int(r) + int(i) * int(i) for r, i in iq]

    def nearest_f32(v):                 # python integers: round v to 24 significant bits, ties to even
        e = max(v.bit_length() - 24, 0)
        q, r = v >> e, v & ((1 << e) - 1)
        half = (1 << e) >> 1
        q += 1 if e and (r > half or (r == half and q & 1)) else 0
        return np.float32(q << e)

    for W in WIDTHS:
        peak, power, exact = frames.trace_of_frame(fb, W)
        P = N // W
        assert peak.shape == power.shape == exact.shape == (P,)
        assert peak.dtype == np.float32 and power.dtype == np.float32 and exact.dtype == np.int64
        assert np.array_equal(peak.view(np.uint32), mag.reshape(P, W).max(axis=1).view(np.uint32))
        want = [sum(ip[j * W:(j + 1) * W]) for j in range(P)]
        assert exact.tolist() == want
        assert np.array_equal(power.view(np.uint32), np.array([nearest_f32(v) for v in want], np.float32).view(np.uint32))
    zero = frames.trace_of_frame(bytes(65536), 16)
    assert not zero[0].view(np.uint32).any() and not zero[1].view(np.uint32).any() and not zero[2].any()
    for bad in (0, 1, 3, 12, 128, -2, 16.0, "16", None, True):
        with pytest.raises(ValueError):
            frames.trace_of_frame(fb, bad)
    with pytest.raises(ValueError):
        frames.trace_of_frame(fb[:-1], 16)


def test_nearest_float32_of_large_sums():
    """numpy's int64 -> float32 conversion, which trace_of_frame and the GPU tests rely on, rounds to nearest even up to
    the defined worst case 2^37."""
    v = np.array([(1 << 24) + 1, (1 << 24) + 3, (1 << 25) + 2, (1 << 25) + 6, (1 << 37) - 1, (1 << 36) + (1 << 12)], np.int64)
    want = [1 << 24, (1 << 24) + 4, 1 << 25, (1 << 25) + 8, 1 << 37, 1 << 36]
    assert v.astype(np.float32).astype(np.int64).tolist() == want


def test_wrapper_refuses_bad_buckets_before_touching_the_device(hip_lib_built):
    """``bucket`` is checked first: no handle, no tensor and no GPU are needed to be told that a width is wrong; and
    process_q15 does not take the trace under any name."""
    from fpga_real_time_fft_analyzer_amd.abi import SA_EINVAL, SpecanError
    from fpga_real_time_fft_analyzer_amd.chain import SpectrumChain
    ch = SpectrumChain.__new__(SpectrumChain)            # no sa_create: there may be no device
    for bad in (0, 1, 3, 12, 65, 128, -16, 16.0, "16", None, True, (16,)):
        with pytest.raises(SpecanError) as e:
            ch.traces_q15(None, bucket=bad)
        assert e.value.code == SA_EINVAL, bad
    for kind in ("trace", 16, 17, 20):
        with pytest.raises(SpecanError) as e:
            ch.process_q15(None, out_kind=kind)
        assert e.value.code == SA_EINVAL, kind
    assert hip_lib_built.sa_process_q15_out(None, None, None, 1, 20, None) == SA_EINVAL
    assert hip_lib_built.sa_process_q15_p12(None, None, None, 1, 20, None) == SA_EINVAL


def test_shape_table():
    import torch
    from fpga_real_time_fft_analyzer_amd import chain
    for W in WIDTHS:
        for B in (0, 1, 5):
            assert chain.output_spec(chain.Q15_TRACE_CHAIN, W, B) == ((B, N // W, 2), torch.float32)
    from fpga_real_time_fft_analyzer_amd.abi import SA_EINVAL, SpecanError
    for bad in (1, 128, "16"):
        with pytest.raises(SpecanError) as e:
            chain.output_spec(chain.Q15_TRACE_CHAIN, bad, 1)
        assert e.value.code == SA_EINVAL
