"""GPU: the float chain on packed 12-bit samples (sa_process_f32_p12; the format is defined in include/specan.h).

The criterion throughout is torch.equal against process_f32 on the int16 tensor of the same samples: the packed entry
point unpacks in the stage-in and then IS the int16 path, so there are no tolerances.  (The int16 path's own parity
with the float32 path and the oracle is pinned by test_gpu_f32.py::test_int16_samples_take_the_float_path_bit_for_bit.)"""
import functools

import numpy as np
import pytest

from conftest import N
from gpu_support import ch, check_overlap_profiling_and_graph_capture, to_device, torch_mod  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

P12 = 24576
KINDS = ("mag_full", "mag_half", "spec_half", "time", "marker")
SCALES = (1.0 / 2048.0, 3.1e-4)


@functools.lru_cache(maxsize=None)
def batch():
    """(int16 [5,N], packed uint8 [5,24576]) of the same samples, read-only:
    0 random; 1 the alternating extremes; 2 the ramp (37 n mod 4096) - 2048, on which a misplaced sample shows;
    3 zero except single samples at the seams of the stage-in (10 and 21 straddle a 16-byte unit, 63 / 64 a thread's
    row, 8191 / 8192 the two halves of the frame); 4 zero."""
    from fpga_real_time_fft_analyzer_amd.ingest import pack12
    rng = np.random.default_rng(2024)
    n = np.arange(N)
    x = np.zeros((5, N), np.int16)
    x[0] = rng.integers(-2048, 2048, N)
    x[1] = np.where(n & 1, 2047, -2048)
    x[2] = (37 * n) % 4096 - 2048
    for k, pos in enumerate((0, 1, 10, 11, 21, 63, 64, 8191, 8192, 16382, 16383)):
        x[3, pos] = (-1) ** k * (100 + 150 * k)
    p = pack12(x)
    assert p.shape == (5, P12)
    x.setflags(write=False)
    p.setflags(write=False)
    return x, p


def cascades():
    from scipy import signal
    return {"none": None, "butter12": signal.butter(12, 0.2, output="sos"),            # 6 sections
            "cheby7": signal.cheby1(7, 1.0, 0.3, output="sos"),                        # 4 sections
            "butter3": signal.butter(3, 0.4, output="sos"),                            # 2 sections
            "default": "0x00"}


def select(ch, sos):
    if sos is None:
        ch.set_filter_mode(0xB1)
    elif isinstance(sos, str):
        ch.set_filter_mode(0x00)
    else:
        ch.load_sos(sos)
        ch.set_filter_mode(0xA1)


def same(torch, a, b):
    if a.is_complex():
        a, b = torch.view_as_real(a), torch.view_as_real(b)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("window", ["hann", "blackman"])
def test_packed_equals_int16_for_every_mode_and_kind(ch, torch_mod, window, scale):
    torch = torch_mod
    x, p = batch()
    d_i, d_p = to_device(torch, x), to_device(torch, p)
    if window == "blackman":
        ch.set_window_f32(np.blackman(N).astype(np.float32))       # a table window: no in-place generator
    for name, sos in cascades().items():
        select(ch, sos)
        for kind in KINDS:
            a = ch.process_f32(d_p, out_kind=kind, scale=scale)
            b = ch.process_f32(d_i, out_kind=kind, scale=scale)
            assert same(torch, a, b), (name, kind)
            if kind == "mag_full":
                assert b[:4].any() and not a[4].any()              # the comparison is not between two empty results


@pytest.mark.parametrize("scale", SCALES)
def test_packed_equals_int16_with_float64_state(ch, torch_mod, scale):
    torch = torch_mod
    x, p = batch()
    d_i, d_p = to_device(torch, x), to_device(torch, p)
    ch.set_precision("f64")
    for window in (None, np.blackman(N).astype(np.float32)):
        if window is not None:
            ch.set_window_f32(window)
        for name in ("butter12", "cheby7", "butter3", "default"):
            select(ch, cascades()[name])
            for kind in ("mag_full", "time"):
                a = ch.process_f32(d_p, out_kind=kind, scale=scale)
                b = ch.process_f32(d_i, out_kind=kind, scale=scale)
                assert same(torch, a, b) and b.any(), (name, kind, window is not None)


def test_sample_order_against_numpy(ch, torch_mod):
    """An order check that does not go through the int16 kernel's stage-in: with a window of ones and no cascade the
    'time' output is x[n] = float32(s[n]) * scale, rounded once, times the chain's constant factor c (the folded 1/2 of
    the window table and the 2 that undoes it: powers of two, so the product is exact and the comparison is equality).
    c is read off the int16 path on a frame that holds one sample."""
    from fpga_real_time_fft_analyzer_amd.ingest import unpack12
    torch = torch_mod
    x, p = batch()
    ch.set_window_f32(np.ones(N, np.float32))
    ch.set_filter_mode(0xB1)
    one = np.zeros((1, N), np.int16)
    one[0, 5] = 1
    c = ch.process_f32(to_device(torch, one), out_kind="time", scale=1.0).cpu().numpy()
    assert c[0, 5] != 0 and not np.delete(c[0], 5).any()
    c = np.float32(c[0, 5])
    for scale in SCALES:
        got = ch.process_f32(to_device(torch, p), out_kind="time", scale=scale).cpu().numpy()
        want = (unpack12(p).astype(np.float32) * np.float32(scale)) * c
        assert want.dtype == np.float32 and np.array_equal(got, want)
        assert np.array_equal(unpack12(p), x)


@pytest.mark.parametrize("mode", ["none", "butter12"])
def test_frame_stride_and_isolation(ch, torch_mod, mode):
    """B = 1, each frame alone, and a whole-frame slice of a larger tensor (its data pointer is offset by whole frames)
    give the rows of the batch call."""
    torch = torch_mod
    _, p = batch()
    d_p = to_device(torch, p)
    select(ch, cascades()[mode])
    for kind in ("mag_full", "time", "marker"):
        ref = ch.process_f32(d_p, out_kind=kind).clone()
        for f in range(5):
            assert torch.equal(ch.process_f32(d_p[f:f + 1].clone(), out_kind=kind), ref[f:f + 1]), (kind, f)
        big = torch.full((7, P12), 0x5A, dtype=torch.uint8, device="cuda")
        big[2:5] = d_p[1:4]
        part = big[2:5]
        assert part.is_contiguous() and part.data_ptr() == big.data_ptr() + 2 * P12
        assert torch.equal(ch.process_f32(part, out_kind=kind), ref[1:4]), kind


def test_marker_range_that_cuts_the_spectrum(ch, torch_mod):
    torch = torch_mod
    x, p = batch()
    d_i, d_p = to_device(torch, x), to_device(torch, p)
    ch.set_marker_range(100, 5000)
    for name in ("none", "butter12"):
        select(ch, cascades()[name])
        rec_p, rec_i = ch.process_f32(d_p, out_kind="marker"), ch.process_f32(d_i, out_kind="marker")
        assert torch.equal(rec_p, rec_i), name
        _, peak_bin, _ = ch.markers(d_p)
        assert ((peak_bin >= 100) & (peak_bin < 5000)).all()


def test_overlap_profiling_and_graph_capture(ch, torch_mod):
    """Everything that holds for the int16 entry point's launches: overlap depth 2 with flush, one device time per timed
    call, and capture into a graph after reserve; all outputs equal the plain stream-ordered call."""
    torch = torch_mod
    _, p = batch()
    d_p = to_device(torch, p)
    select(ch, cascades()["butter12"])
    ch.reserve(8)
    ref = ch.process_f32(d_p).clone()
    check_overlap_profiling_and_graph_capture(torch, ch, lambda out: ch.process_f32(d_p, out=out), ref)


def test_argument_errors(ch, torch_mod):
    from fpga_real_time_fft_analyzer_amd.abi import SA_EINVAL, SA_ESHAPE, SA_ESTATE, SpecanError
    torch = torch_mod
    _, p = batch()
    d_p = to_device(torch, p[:2])
    ref = ch.process_f32(d_p).clone()
    flat = torch.zeros(8 + 2 * P12, dtype=torch.uint8, device="cuda")
    off = flat[8:].view(2, P12)                                    # contiguous, 8 bytes off a 16-byte boundary
    off.copy_(d_p)
    assert off.is_contiguous() and off.data_ptr() % 16 == 8
    with pytest.raises(SpecanError) as e:
        ch.process_f32(off)
    assert e.value.code == SA_EINVAL
    assert torch.equal(ch.process_f32(d_p), ref)                   # nothing was launched, no call state changed
    with pytest.raises(SpecanError) as e:
        ch.process_f32(d_p, scale=float("nan"))
    assert e.value.code == SA_EINVAL
    with pytest.raises(SpecanError) as e:
        ch.process_f32(torch.zeros((2, P12 - 1), dtype=torch.uint8, device="cuda"))
    assert e.value.code == SA_ESHAPE
    ch.set_filter_mode(0xA2)
    with pytest.raises(SpecanError) as e:
        ch.process_f32(d_p)
    assert e.value.code == SA_ESTATE
    ch.set_filter_mode(0xB1)
    assert torch.equal(ch.process_f32(d_p), ref)


def test_packed_feeder_gives_the_int16_feeders_outputs(ch, torch_mod):
    from fpga_real_time_fft_analyzer_amd.ingest import DeviceFeeder, FrameCutter, pack12
    torch = torch_mod
    rng = np.random.default_rng(77)
    stream = rng.integers(-2048, 2048, 10 * N + 123).astype(np.int16)
    hop = 8192
    frames_i = FrameCutter(hop).push(stream)                       # 19 frames
    packed = pack12(stream[:stream.size & ~1])
    cutter = FrameCutter(hop, packed=True)
    frames_p = np.concatenate([cutter.push(packed[i:i + 50001]) for i in range(0, packed.size, 50001)])
    assert frames_p.shape == (frames_i.shape[0], P12) and frames_i.shape[0] == 19
    select(ch, cascades()["butter12"])

    def run(feeder, frames):
        got = [ch.process_f32(xd).clone() for xd in feeder.feed(frames[i:i + 8] for i in range(0, len(frames), 8))]
        torch.cuda.synchronize()
        return torch.cat(got)

    out_i = run(DeviceFeeder(0, max_batch=8), frames_i)
    out_p = run(DeviceFeeder(0, max_batch=8, packed=True), frames_p)
    assert out_p.shape == (19, N) and torch.equal(out_p, out_i) and out_i.any()
