"""GPU: the display-trace kinds of the integer chain (include/specan.h, SA_Q15_TRACE_KIND(k): one {peak_mag, power} record
per bucket of W = 2^k bins), through SpectrumChain.traces_q15 and the two C entry points.

Every comparison is exact, on float bits: the records are bit-defined.  The expected values are numpy on the ORACLE's
frames oracle.chain_q15(...): the peak is the bucket maximum of frames.decode_mag_16iq_le, the power the int64 sum of
re^2 + im^2 over the bucket converted once to float32 (nearest even; tests/test_q15_trace_cpu.py pins that conversion).
"""
import numpy as np
import pytest

from conftest import N
from gpu_support import ch, check_overlap_profiling_and_graph_capture, to_device, torch_mod  # noqa: F401 (fixtures)
from q15_cases import SETUP_OF_MODE, configure, extreme_frames, records_equal, uniform
from q15_mirrors import bits as _bits, decode as _decode, trace_expect as _expect

pytestmark = pytest.mark.gpu

WIDTHS = (2, 4, 8, 16, 32, 64)
FORMS = ("b1_rtl", "b1_hann_u16", "b1_rom_rtl", "b1_rom_hann_u16", "default", "gui_upload", "wide2", "wide6_hann_u16")      # of SETUPS


def _check(rec, mag, ip, W, tag=""):
    """a [B,P,2] float32 record tensor against numpy on the decoded frames, by bits"""
    peak, power, _ = _expect(mag, ip, W)
    records_equal(rec, peak, power, (mag.shape[0], N // W, 2), (tag, W))


@pytest.mark.parametrize("form", FORMS)
def test_records_equal_numpy_on_the_oracles_frames(ch, torch_mod, oracle, form):
    """All six widths in filter modes 0xB1 (both window modes, default and custom ROM), 0x00, 0xA1 with the GUI upload and
    0xA2 with 2 and 6 sections; B = 1, 7 and 33; 12-bit and full-scale samples; int16 input and, for the 12-bit samples,
    the packed form of the same samples.  From B = 7 on, frame 1 is all zero: its records have all bits zero."""
    from fpga_real_time_fft_analyzer_amd import frames
    from fpga_real_time_fft_analyzer_amd.ingest import pack12
    rng = np.random.default_rng(1100 + FORMS.index(form))
    args = configure(ch, form, rng)
    for B in (1, 7, 33):
        for full in (False, True):
            x = uniform(rng, (B, N), full)
            if B >= 7:
                x[1] = 0
            ref = oracle.chain_q15(x, *args)
            mag, ip = _decode(ref)
            assert mag.any()
            xd = to_device(torch_mod, x)
            pd = None if full else to_device(torch_mod, pack12(x))
            for W in WIDTHS:
                rec = ch.traces_q15(xd, bucket=W)
                _check(rec, mag, ip, W, (form, B, full, "int16"))
                if pd is not None:
                    _check(ch.traces_q15(pd, bucket=W), mag, ip, W, (form, B, full, "p12"))
                if B >= 7:
                    assert not ref[1].any() and not rec[1].view(torch_mod.int32).any().item(), (form, B, W)
            if B == 1:                                             # the numpy mirror is the same definition
                peak, power, exact = frames.trace_of_frame(ref[0].astype("<i2").tobytes(), 16)
                want = _expect(mag, ip, 16)
                assert np.array_equal(_bits(peak), _bits(want[0][0])) and np.array_equal(_bits(power), _bits(want[1][0]))
                assert np.array_equal(exact, want[2][0])
    # the default bucket is 16
    assert torch_mod.equal(ch.traces_q15(xd), ch.traces_q15(xd, bucket=16))


def test_cross_check_against_mag_and_marker_on_the_same_handle(ch, torch_mod):
    """The trace against the existing kinds of the same handle, no oracle involved: the peak is mag.view(B,P,W).amax(-1) by
    bits; for buckets at lane-row, wave and m' edges (W = 16: j = 0, 1, 3, 4, 63, 64, P-1; W = 64: j = 0, 15, 16, P-1) the
    marker record over [jW, (j+1)W) has the same peak bits and a band_power whose float32 rounding is the trace's power.
    The marker range changes no trace bit."""
    torch = torch_mod
    rng = np.random.default_rng(77)
    x = rng.integers(-32768, 32768, size=(7, N)).astype(np.int16)
    xd = to_device(torch, x)
    ch.set_window_mode_q15(1)
    ch.set_filter_mode(0xB1)
    B = 7
    mag = ch.process_q15(xd, out_kind="mag")
    first = {W: ch.traces_q15(xd, bucket=W).clone() for W in WIDTHS}
    for W in WIDTHS:
        want = mag.view(B, N // W, W).amax(-1)
        assert torch.equal(first[W][..., 0].contiguous().view(torch.int32), want.contiguous().view(torch.int32)), W
    for W, js in ((16, (0, 1, 3, 4, 63, 64, N // 16 - 1)), (64, (0, 15, 16, N // 64 - 1))):
        for j in js:
            ch.set_marker_range(j * W, (j + 1) * W)
            pm, pb, bp = ch.markers_q15(xd)
            tr = ch.traces_q15(xd, bucket=W)
            assert torch.equal(tr, first[W]), (W, j)                       # the range changed nothing
            t = tr.cpu().numpy()
            assert np.array_equal(_bits(pm.cpu().numpy()), _bits(t[:, j, 0])), (W, j)
            assert ((pb.cpu().numpy() >= j * W) & (pb.cpu().numpy() < (j + 1) * W)).all()
            assert np.array_equal(_bits(bp.cpu().numpy().astype(np.float32)), _bits(t[:, j, 1])), (W, j)
    ch.set_marker_range(5, 6)
    for W in WIDTHS:
        assert torch.equal(ch.traces_q15(xd, bucket=W), first[W]), W


def two_tone_batch():
    """48 frames of two tones of amplitude 0.3 .. 0.5 of full scale each, random bins in [16, 8176) and phases; every
    third frame's tones sit off the bin grid.  Their sum stays inside int16."""
    rng = np.random.default_rng(4)
    n = np.arange(N)
    x = np.zeros((48, N), np.int16)
    for f in range(48):
        s = np.zeros(N)
        for _ in range(2):
            b = float(rng.integers(16, 8176)) + (rng.uniform(0.1, 0.9) if f % 3 == 2 else 0.0)
            s += rng.uniform(0.3, 0.5) * 32767.0 * np.cos(2 * np.pi * b * n / N + rng.uniform(0, 2 * np.pi))
        x[f] = np.rint(s).astype(np.int16)
    return x


def rounding_counts(ip, W):
    """On exact integer powers [B,N]: the number of buckets whose sum rounds differently toward zero than to nearest, and
    the number whose left-to-right float32 accumulation of the per-bin powers differs from the rounded exact sum."""
    B = ip.shape[0]
    exact = ip.reshape(B, N // W, W).sum(axis=2)
    rne = exact.astype(np.float32)
    rtz = np.where(rne.astype(np.int64) > exact, np.nextafter(rne, np.float32(0)), rne)
    acc = np.zeros_like(rne)
    terms = ip.reshape(B, N // W, W).astype(np.float32)
    for i in range(W):
        acc = (acc + terms[..., i]).astype(np.float32)
    return int((_bits(rtz) != _bits(rne)).sum()), int((_bits(acc) != _bits(rne)).sum())


def test_rounding_is_exercised(ch, torch_mod, oracle):
    """One rounding of an exact sum, really tested: on 48 two-tone frames (mode 0xB1, the 16-bit Hann window mode) the
    reference alone must show, before the GPU is asked, for every W at least 10 buckets whose sum rounds differently
    toward zero than to nearest, and for every W >= 4 at least 5 buckets where a left-to-right float32 accumulation gives
    another float (at W = 2 a two-term float sum is correctly rounded whenever both terms are exact floats).  Measured on
    the oracle's frames for W = 2 .. 64: 17, 19, 21, 25, 25, 22 buckets under round-toward-zero and 0, 12, 33, 54, 72, 77
    under float32 accumulation."""
    x = two_tone_batch()
    ref = oracle.chain_q15(x, None, 1, 0xB1, None, None)
    mag, ip = _decode(ref)
    for W in WIDTHS:
        n_rtz, n_acc = rounding_counts(ip, W)
        print(f"FIGURE rounding cases at W = {W}: {n_rtz} buckets differ under round-toward-zero, {n_acc} under float32 accumulation")
        assert n_rtz >= 10, (W, n_rtz)
        assert W < 4 or n_acc >= 5, (W, n_acc)
    ch.set_window_mode_q15(1)
    ch.set_filter_mode(0xB1)
    xd = to_device(torch_mod, x)
    for W in WIDTHS:
        _check(ch.traces_q15(xd, bucket=W), mag, ip, W, "two tones")


def test_extreme_frames(ch, torch_mod, oracle):
    """Constant +32767, constant -32768, alternating extremes, a lone -32768 impulse and all zero: in modes 0xB1 and 0x00
    under the default ROM, and through a saturating section in mode 0xA2 under a constant ROM (b0 = 32767 in Q2.14: the
    constant frames leave the cascade at the rails), where the oracle's frames hold a component of -32768 -- asserted, so
    the 2^30 square cannot go missing.  The zero frame's records have all bits zero."""
    x = extreme_frames(zero_frame=True)
    xd = to_device(torch_mod, x)
    sat =np.array([[32767, 0, 0, 16384, 0, 0]], np.int16)
    ch.load_sos_q14(sat)
    reached = 0
    for cmd, rom_v in ((0xB1, None), (0x00, None), (0xA2, -32768), (0xA2, 32767)):
        rom = None if rom_v is None else np.full(N, rom_v, np.int16)
        ch.set_window_q15(rom)
        ch.set_filter_mode(cmd)
        ref = oracle.chain_q15(x, rom, 0, cmd, None, sat)
        reached += int((ref == -32768).sum())
        mag, ip = _decode(ref)
        assert not ref[4].any()
        for W in WIDTHS:
            rec = ch.traces_q15(xd, bucket=W)
            _check(rec, mag, ip, W, (hex(cmd), rom_v))
            assert not rec[4].view(torch_mod.int32).any().item(), (hex(cmd), W)
    assert reached >= 1, reached


def test_bounds_and_frame_isolation(ch, torch_mod, oracle):
    """B = 5, every width: `out` sits inside a larger canary-filled tensor and nothing outside [B,P,2] changes; permuting
    the batch permutes the records."""
    torch = torch_mod
    rng = np.random.default_rng(55)
    x = rng.integers(-2048, 2048, size=(5, N)).astype(np.int16)
    ch.set_filter_mode(0x00)
    mag, ip = _decode(oracle.chain_q15(x, None, 0, 0x00, None, None))
    xd = to_device(torch, x)
    perm = [3, 0, 4, 2, 1]
    xp = to_device(torch, x[perm])
    canary = 0x7FC0BEEF                                      # a NaN pattern no record can hold
    pad = 4096                                               # floats: keeps the embedded tensor 16-byte aligned
    for W in WIDTHS:
        n = 5 * (N // W) * 2
        big = torch.full((n + 2 * pad,), canary, dtype=torch.int32, device="cuda")
        out = big[pad:pad + n].view(torch.float32).view(5, N // W, 2)
        assert out.data_ptr() % 16 == 0
        got = ch.traces_q15(xd, bucket=W, out=out)
        assert got.data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        assert (big[:pad] == canary).all().item() and (big[pad + n:] == canary).all().item(), W
        _check(out, mag, ip, W, "embedded")
        assert torch.equal(ch.traces_q15(xp, bucket=W), out[perm]), W


@pytest.mark.parametrize("mode", ["0xB1", "0x00", "0xA2", "0xB1-p12", "0xA2-p12"])
def test_overlap_profiling_and_graph_capture(ch, torch_mod, oracle, mode):
    """The trace in the unstaged launch (0xB1) and the staged one (0x00, 0xA2 with six sections), on int16 and packed
    input: overlap depth 2 with flush, one device time per timed call, capture into a graph; identical records across
    repeated calls, equal to numpy on the oracle's frames."""
    from fpga_real_time_fft_analyzer_amd.ingest import pack12
    torch = torch_mod
    cmd = int(mode[:4], 16)
    rng = np.random.default_rng(66)
    x = rng.integers(-2048, 2048, size=(9, N)).astype(np.int16)
    args = configure(ch, SETUP_OF_MODE[cmd])
    ch.reserve(9)
    mag, ip = _decode(oracle.chain_q15(x, *args))
    xd = to_device(torch, pack12(x) if mode.endswith("p12") else x)
    for W in (16, 64):
        ref = ch.traces_q15(xd, bucket=W).clone()
        _check(ref, mag, ip, W, mode)
        for _ in range(3):
            assert torch.equal(ch.traces_q15(xd, bucket=W), ref), (mode, W)
        check_overlap_profiling_and_graph_capture(torch, ch, lambda o: ch.traces_q15(xd, bucket=W, out=o), ref)


def test_refusals_leave_the_handle_usable(ch, torch_mod, oracle):
    """Through both C entry points: kinds 16, 23 and 3, an `out` 8 bytes off a 16-byte boundary, NULL in and NULL out are
    SA_EINVAL; the profiling ring shows no launch for them; a good call afterwards is correct.  sa_process_f32 refuses
    kind 17.  The wrapper refuses a wrong `out`."""
    from fpga_real_time_fft_analyzer_amd import abi
    from fpga_real_time_fft_analyzer_amd.abi import SA_EINVAL, SA_ESHAPE, SpecanError
    from fpga_real_time_fft_analyzer_amd.ingest import pack12
    torch = torch_mod
    rng = np.random.default_rng(13)
    x = rng.integers(-2048, 2048, size=(4, N)).astype(np.int16)
    ch.set_filter_mode(0x00)
    mag, ip = _decode(oracle.chain_q15(x, None, 0, 0x00, None, None))
    xd, pd = to_device(torch, x), to_device(torch, pack12(x))
    L = abi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    W, kind = 16, abi.SA_Q15_TRACE_KIND(4)
    out = torch.zeros((4, N // W, 2), dtype=torch.float32, device="cuda")
    ch.set_profiling(64)
    assert L.sa_process_q15_out(ch._h, xd.data_ptr(), out.data_ptr(), 4, kind, stream) == 0
    assert L.sa_process_q15_p12(ch._h, pd.data_ptr(), out.data_ptr(), 4, kind, stream) == 0
    timed = len(ch.profile_read(64))
    assert timed == 2
    for fn, d in ((L.sa_process_q15_out, xd), (L.sa_process_q15_p12, pd)):
        for bad in (16, 23, 3):
            assert fn(ch._h, d.data_ptr(), out.data_ptr(), 4, bad, stream) == SA_EINVAL, bad
        assert fn(ch._h, d.data_ptr(), out.data_ptr() + 8, 3, kind, stream) == SA_EINVAL
        assert fn(ch._h, None, out.data_ptr(), 4, kind, stream) == SA_EINVAL
        assert fn(ch._h, d.data_ptr(), None, 4, kind, stream) == SA_EINVAL
    xf = torch.zeros((4, N), dtype=torch.float32, device="cuda")
    of = torch.zeros((4, N), dtype=torch.float32, device="cuda")
    assert L.sa_process_f32(ch._h, xf.data_ptr(), of.data_ptr(), 4, abi.SA_Q15_TRACE_KIND(1), stream) == SA_EINVAL
    assert len(ch.profile_read(64)) == timed        # no refused call was timed: no call state committed
    ch.set_profiling(0)
    out.zero_()
    assert L.sa_process_q15_out(ch._h, xd.data_ptr(), out.data_ptr(), 4, kind, stream) == 0
    _check(out, mag, ip, W, "after refusals")
    out.zero_()
    assert L.sa_process_q15_p12(ch._h, pd.data_ptr(), out.data_ptr(), 4, kind, stream) == 0
    _check(out, mag, ip, W, "after refusals, p12")
    for bad_out in (torch.empty((4, N // W, 2), dtype=torch.int32, device="cuda"),
                    torch.empty((4, N // 8, 2), dtype=torch.float32, device="cuda")):
        with pytest.raises(SpecanError) as e:
            ch.traces_q15(xd, bucket=W, out=bad_out)
        assert e.value.code == SA_ESHAPE
    _check(ch.traces_q15(xd, bucket=W), mag, ip, W, "after wrapper refusals")
    e = torch.empty((0, N), dtype=torch.int16, device="cuda")
    assert ch.traces_q15(e, bucket=64).shape == (0, N // 64, 2)
