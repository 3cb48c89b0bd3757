"""GPU: the grouped trace kinds of the integer chain (include/specan.h, SA_Q15_TRACE_AVG_KIND(k, a): one {peak_mag, power}
record per bucket of W = 2^k bins and group of A = 2^a consecutive frames -- max hold and summed power), through
SpectrumChain.traces_q15(group=A) and the two C entry points.

Every comparison is exact, on float bits.  The reference is the call the kind derives from: the handle's own
process_q15(..., out_kind="iq") on the same input, reduced in numpy in int64 -- the peak is the maximum over bucket and group
of frames.decode_mag_16iq_le, the power the int64 sum of re^2 + im^2 over bucket and group converted once to float32 (nearest
even; tests/test_q15_trace_avg_cpu.py pins that conversion up to 2^44).  The first test holds those frames to the oracle's
too."""
import numpy as np
import pytest

from conftest import N
from gpu_support import ch, check_overlap_profiling_and_graph_capture, to_device, torch_mod  # noqa: F401 (fixtures)
from fpga_real_time_fft_analyzer_amd.abi import SA_EINVAL, SA_ESHAPE, SA_ESTATE
from q15_cases import SETUP_OF_MODE, SETUPS, configure, handle_iq as _iq, records_equal, uniform
from q15_mirrors import bits as _bits, decode as _decode, trace_expect as _expect

pytestmark = pytest.mark.gpu

WIDTHS = (2, 4, 8, 16, 32, 64)
BAD_WORDS = (0x80, 0x81, 0x86, 0x88, 0x8F, 0xC9)
FORMS = ("b1_rtl", "b1_rom_hann_u16", "default", "gui_upload", "wide6")       # of q15_cases.SETUPS
SHAPES = ((2, 2), (2, 6), (4, 8), (8, 24))                   # (A, B): every B is a prefix of one 24-frame batch


def _check(rec, mag, ip, W, A, tag=""):
    """a [B/A,P,2] float32 record tensor against numpy on the decoded frames, by bits"""
    peak, power, _ = _expect(mag, ip, W, A)
    records_equal(rec, peak, power, (mag.shape[0] // A, N // W, 2), (tag, W, A))


@pytest.mark.parametrize("form", FORMS)
def test_records_equal_numpy(ch, torch_mod, oracle, form):
    """Modes 0xB1 (RTL window; a custom ROM in the 16-bit Hann mode), 0x00, 0xA1 with the GUI upload and 0xA2 with six
    sections; (A, B) = (2,2), (2,6), (4,8), (8,24) at all six widths -- the first B frames of one 24-frame batch whose frames 2
    and 3 are zero, so that in (2,6) group 1 is all zero: its records have all bits zero, and its neighbours are what the
    reference says; 12-bit samples as int16 and packed, and full-scale int16.  In 0xB1 also (128,128) and (128,256) at W = 2
    and 64.  The handle's IQ frames, the reference, are the oracle's for the 24-frame batches."""
    from fpga_real_time_fft_analyzer_amd.ingest import pack12
    torch = torch_mod
    rng = np.random.default_rng(1300 + FORMS.index(form))
    args = configure(ch, form, rng)
    for full in (False, True):
        x = uniform(rng, (24, N), full)
        x[2:4] = 0
        xd = to_device(torch, x)
        pd = None if full else to_device(torch, pack12(x))
        ref = _iq(ch, xd)
        assert np.array_equal(ref, oracle.chain_q15(x, *args)), (form, full)
        mag, ip = _decode(ref)
        assert mag[:2].any() and not ref[2:4].any()
        for A, B in SHAPES:
            for W in WIDTHS:
                tag = (form, full, A, B)
                rec = ch.traces_q15(xd[:B], bucket=W, group=A)
                _check(rec, mag[:B], ip[:B], W, A, tag + ("int16",))
                if pd is not None:
                    _check(ch.traces_q15(pd[:B], bucket=W, group=A), mag[:B], ip[:B], W, A, tag + ("p12",))
                if (A, B) == (2, 6):
                    assert not rec[1].view(torch.int32).any().item(), tag
                    assert rec[0].view(torch.int32).any().item() and rec[2].view(torch.int32).any().item(), tag
    if SETUPS[form].cmd != 0xB1 or SETUPS[form].custom_rom:
        return
    for full in (False, True):
        x = uniform(rng, (256, N), full)
        xd = to_device(torch, x)
        pd = None if full else to_device(torch, pack12(x))
        mag, ip = _decode(_iq(ch, xd))
        for B in (128, 256):
            for W in (2, 64):
                _check(ch.traces_q15(xd[:B], bucket=W, group=128), mag[:B], ip[:B], W, 128, (form, full, B, "int16"))
                if pd is not None:
                    _check(ch.traces_q15(pd[:B], bucket=W, group=128), mag[:B], ip[:B], W, 128, (form, full, B, "p12"))


@pytest.mark.parametrize("cmd", [0xB1, 0x00])
def test_group_edges(ch, torch_mod, cmd):
    """A = 4, B = 8, batches in which only the first (or only the last) frame of each group is non-zero: a full-scale frame
    in group 0, a frame of amplitude <= 16 in group 1.  Each group's records are the single frame's plain trace -- the same
    maximum, and the same exact sum rounded the same once, so by bits at every power (asserted to lie below 2^24 for the
    small frame and, in mode 0xB1, to pass it for the large one) -- and the int64 reference's.  Nothing leaks across the group boundary."""
    torch = torch_mod
    rng = np.random.default_rng(31)
    ch.set_filter_mode(cmd)
    n = np.arange(N)                                           # a tone near full scale (in 0xB1: 4.8e7 of power in its bin) and noise
    big = (np.rint(28000 * np.cos(2 * np.pi * 1000 * n / N)) + rng.integers(-4000, 4001, size=N)).astype(np.int16)
    # two tones of amplitude 7 and a last bit of noise: |x| <= 16
    small = (np.rint(7 * np.cos(2 * np.pi * 100 * n / N) + 7 * np.cos(2 * np.pi * 6000 * n / N)) + rng.integers(-1, 2, size=N)).astype(np.int16)
    assert np.abs(small).max() <= 16
    for pos in (0, 3):
        x = np.zeros((8, N), np.int16)
        x[pos], x[4 + pos] = big, small
        xd = to_device(torch, x)
        mag, ip = _decode(_iq(ch, xd))
        assert mag[pos].any() and mag[4 + pos].any() and not mag[[i for i in range(8) if i % 4 != pos]].any()
        for W in (2, 16, 64):
            rec = ch.traces_q15(xd, bucket=W, group=4)
            _check(rec, mag, ip, W, 4, (hex(cmd), pos))
            plain = ch.traces_q15(xd, bucket=W)
            assert torch.equal(rec[0].view(torch.int32), plain[pos].view(torch.int32)), (hex(cmd), pos, W)
            assert torch.equal(rec[1].view(torch.int32), plain[4 + pos].view(torch.int32)), (hex(cmd), pos, W)
            assert 0.0 < plain[4 + pos, :, 1].max().item() < float(1 << 24), (hex(cmd), pos, W)
            if cmd == 0xB1:                                    # the default cascade leaves the tone below 2^10
                assert plain[pos, :, 1].max().item() >= float(1 << 24), (hex(cmd), pos, W)


@pytest.mark.parametrize("A", [8, 32, 128])
def test_carry_and_rounding_on_the_device(ch, torch_mod, A):
    """Mode 0xB1 under a ROM of all 32767: a constant +32767 frame puts about 2^30 of power into bin 0.  B = 2 A: three
    quarters of group 0 are such frames, the rest of the batch random full-scale frames, which populate the low-order
    bits.  The reference's own largest sum is asserted to exceed 2^32 (A = 8), 2^34 (A = 32) and 2^36 (A = 128) before
    the bits are compared, at W = 2 and 64."""
    torch = torch_mod
    rng = np.random.default_rng(40 + A)
    ch.set_window_q15(np.full(N, 32767, np.int16))
    ch.set_filter_mode(0xB1)
    x = rng.integers(-32768, 32768, size=(2 * A, N)).astype(np.int16)
    x[:3 * A // 4] = 32767
    xd = to_device(torch, x)
    mag, ip = _decode(_iq(ch, xd))
    assert ip[0, 0] > 0.99 * 2 ** 30
    for W in (2, 64):
        _, power, exact = _expect(mag, ip, W, A)
        floor = {8: 1 << 32, 32: 1 << 34, 128: 1 << 36}[A]
        print(f"FIGURE A = {A}, W = {W}: largest exact sum {int(exact.max())} = 2^{np.log2(float(exact.max())):.3f}")
        assert exact.max() > floor and exact[0, 0] == exact.max(), (A, W, int(exact.max()))
        assert (power.astype(np.float64) != exact).any()            # the rounding is a real one somewhere
        _check(ch.traces_q15(xd, bucket=W, group=A), mag, ip, W, A, ("carry", A))


def test_against_the_existing_kinds(ch, torch_mod):
    """No host reference: the peak is the plain trace's peaks of the same handle, maximum over each group, by bits (every
    width, A = 2 and 4); at (A, B) = (2, 4), W = 16 and j = 0, 1, 63, 64, P - 1 the two frames' marker band_power over
    [jW, (j+1)W), added as integers and rounded once to float32, is the record's power.  The marker range changes no bit."""
    torch = torch_mod
    rng = np.random.default_rng(78)
    x = rng.integers(-32768, 32768, size=(4, N)).astype(np.int16)
    xd = to_device(torch, x)
    ch.set_window_mode_q15(1)
    ch.set_filter_mode(0xB1)
    first = {}
    for W in WIDTHS:
        plain = ch.traces_q15(xd, bucket=W)[..., 0].contiguous()
        for A in (2, 4):
            rec = ch.traces_q15(xd, bucket=W, group=A).clone()
            first[W, A] = rec
            want = plain.view(4 // A, A, N // W).amax(1)
            assert torch.equal(rec[..., 0].contiguous().view(torch.int32), want.contiguous().view(torch.int32)), (W, A)
    W, P = 16, N // 16
    for j in (0, 1, 63, 64, P - 1):
        ch.set_marker_range(j * W, (j + 1) * W)
        _, _, bp = ch.markers_q15(xd)
        rec = ch.traces_q15(xd, bucket=W, group=2)
        assert torch.equal(rec, first[W, 2]), j                                    # the range changed nothing
        total = bp.cpu().numpy().astype(np.int64).reshape(2, 2).sum(axis=1)
        assert np.array_equal(_bits(total.astype(np.float32)), _bits(rec[:, j, 1].cpu().numpy())), j
    ch.set_marker_range(5, 6)
    for (W, A), rec in first.items():
        assert torch.equal(ch.traces_q15(xd, bucket=W, group=A), rec), (W, A)


@pytest.mark.parametrize("hop", [8, 4104, 8192])
def test_hop_streams(ch, torch_mod, hop):
    """One sample stream, int16 and packed, cut on the device: (A, B) = (2,4) and (4,8) equal the frame call on the frames
    cut on the host, in mode 0xB1 (the FFT reads the stream) and 0x00 (the cascade does), and both equal the reference."""
    from fpga_real_time_fft_analyzer_amd.ingest import pack12
    torch = torch_mod
    rng = np.random.default_rng(hop)
    for cmd in (0xB1, 0x00):
        ch.set_filter_mode(cmd)
        for A, B in ((2, 4), (4, 8)):
            s = rng.integers(-2048, 2048, size=(B - 1) * hop + N).astype(np.int16)
            fr = np.stack([s[i * hop:i * hop + N] for i in range(B)])
            sd, fd = to_device(torch, s), to_device(torch, fr)
            sp, fp = to_device(torch, pack12(s)), to_device(torch, pack12(fr))
            mag, ip = _decode(_iq(ch, fd))
            for W in (2, 16):
                want = ch.traces_q15(fd, bucket=W, group=A)
                _check(want, mag, ip, W, A, (hop, hex(cmd)))
                assert torch.equal(ch.traces_q15(sd, bucket=W, group=A, hop=hop), want), (hop, hex(cmd), A, W)
                assert torch.equal(ch.traces_q15(sp, bucket=W, group=A, hop=hop), want), (hop, hex(cmd), A, W, "p12")
                assert torch.equal(ch.traces_q15(fp, bucket=W, group=A), want), (hop, hex(cmd), A, W, "p12 frames")


@pytest.mark.parametrize("cmd", [0xB1, 0x00, 0xA2])
def test_overlap_profiling_and_graph_capture(ch, torch_mod, cmd):
    """The grouped call in the unstaged launch (0xB1: FFT, fold) and the staged one (0x00, 0xA2 with six sections: cascade,
    FFT, fold): overlap depth 2 with flush, one device time per timed call, capture into a graph; identical records across
    repeated calls, equal to the reference.  The reference call is the warm-up that grows slot 0's workspaces."""
    torch = torch_mod
    rng = np.random.default_rng(67)
    x = rng.integers(-2048, 2048, size=(8, N)).astype(np.int16)
    configure(ch, SETUP_OF_MODE[cmd])
    xd = to_device(torch, x)
    mag, ip = _decode(_iq(ch, xd))
    for W, A in ((16, 4), (64, 2)):
        ref = ch.traces_q15(xd, bucket=W, group=A).clone()
        _check(ref, mag, ip, W, A, hex(cmd))
        for _ in range(3):
            assert torch.equal(ch.traces_q15(xd, bucket=W, group=A), ref), (hex(cmd), W, A)
        check_overlap_profiling_and_graph_capture(torch, ch, lambda o: ch.traces_q15(xd, bucket=W, group=A, out=o), ref)


def test_capture_with_a_workspace_too_small_is_refused(ch, torch_mod):
    """A fresh handle that has made a (A, B, W) = (4, 8, 16) call holds 8 x 1024 partial records.  Inside a capture, the
    (4, 16, W = 2) call, which needs 16 x 8192, is SA_ESTATE with a message that names the remedy, and nothing of it is
    launched: the graph holds the good call alone, replays it with the right bits, and the handle goes on -- the refused
    call succeeds outside the capture, and is then captured like any other."""
    from fpga_real_time_fft_analyzer_amd.abi import SpecanError
    torch = torch_mod
    rng = np.random.default_rng(68)
    x = rng.integers(-2048, 2048, size=(16, N)).astype(np.int16)
    xd = to_device(torch, x)
    ch.set_filter_mode(0xB1)
    ch.reserve(16)                                                                   # sizes nothing for this kind
    mag, ip = _decode(_iq(ch, xd))
    ref = ch.traces_q15(xd[:8], bucket=16, group=4).clone()
    _check(ref, mag[:8], ip[:8], 16, 4, "warm-up")
    out = torch.zeros_like(ref)
    big = torch.full((4, N // 2, 2), 7.0, dtype=torch.float32, device="cuda")
    graph = torch.cuda.CUDAGraph()
    refused = []
    with torch.cuda.graph(graph):
        ch.traces_q15(xd[:8], bucket=16, group=4, out=out)
        try:
            ch.traces_q15(xd, bucket=2, group=4, out=big)
            refused.append("accepted")
        except SpecanError as e:
            refused.append((e.code, "outside the capture" in str(e)))
    assert refused == [(SA_ESTATE, True)], refused
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    assert (big == 7.0).all().item()                                                 # the refused call wrote nothing
    got = ch.traces_q15(xd, bucket=2, group=4, out=big)                              # grows the workspace
    _check(got, mag, ip, 2, 4, "after the capture")
    graph2 = torch.cuda.CUDAGraph()
    big.zero_()
    with torch.cuda.graph(graph2):
        ch.traces_q15(xd, bucket=2, group=4, out=big)
    big.zero_()
    graph2.replay()
    torch.cuda.synchronize()
    _check(big, mag, ip, 2, 4, "captured after growth")
    assert torch.equal(ch.traces_q15(xd[:8], bucket=16, group=4), ref)
    out.zero_()                                                                      # the first graph reads the workspace it was
    graph.replay()                                                                   # captured with: outgrown, retired, not freed
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


def test_refusals_leave_the_handle_usable(ch, torch_mod):
    """Through both C entry points, into a slice of a canary-filled tensor: good calls change no byte outside
    [out, out + (B / A) P 8); the SA_EINVAL words, an `out` 8 bytes off, NULL in and NULL out, and B = A + 1 (SA_ESHAPE) change
    no byte at all and the profiling ring shows no launch for them; the float entry points refuse 0x9C; a good call
    afterwards is correct.  The wrapper refuses group = 0, 1, 3, 256, 2.0 and True (SA_EINVAL) and B = 6 with group = 4
    (SA_ESHAPE)."""
    from fpga_real_time_fft_analyzer_amd import abi
    from fpga_real_time_fft_analyzer_amd.abi import SpecanError
    from fpga_real_time_fft_analyzer_amd.ingest import pack12
    torch = torch_mod
    rng = np.random.default_rng(14)
    A, B, W = 8, 16, 16
    kind = abi.SA_Q15_TRACE_AVG_KIND(4, 3)
    assert kind == 0x9C
    x = rng.integers(-2048, 2048, size=(B + 1, N)).astype(np.int16)
    ch.set_filter_mode(0x00)
    xd, pd = to_device(torch, x), to_device(torch, pack12(x))
    mag, ip = _decode(_iq(ch, xd[:B]))
    L = abi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    canary, pad = 0x7FC0BEEF, 4096
    n = (B // A) * (N // W) * 2
    bigt = torch.full((n + 2 * pad,), canary, dtype=torch.int32, device="cuda")
    out = bigt[pad:pad + n].view(torch.float32).view(B // A, N // W, 2)
    assert out.data_ptr() % 16 == 0

    def untouched(whole):
        torch.cuda.synchronize()
        ok = (bigt[:pad] == canary).all().item() and (bigt[pad + n:] == canary).all().item()
        return ok and (not whole or (bigt == canary).all().item())

    ch.set_profiling(64)
    calls = ((L.sa_process_q15_out, xd), (L.sa_process_q15_p12, pd))
    for fn, d in calls:
        assert fn(ch._h, d.data_ptr(), out.data_ptr(), B, kind, stream) == 0
        assert untouched(False)
        _check(out, mag, ip, W, A, "good call")
        bigt.fill_(canary)
    timed = len(ch.profile_read(64))
    assert timed == 2
    for fn, d in calls:
        for bad in BAD_WORDS:
            assert fn(ch._h, d.data_ptr(), out.data_ptr(), B, bad, stream) == SA_EINVAL, hex(bad)
            assert fn(ch._h, d.data_ptr(), out.data_ptr(), 0, bad, stream) == SA_EINVAL, hex(bad)
        assert fn(ch._h, d.data_ptr(), out.data_ptr() + 8, B, kind, stream) == SA_EINVAL
        assert b"SA_Q15_TRACE_AVG_KIND" in L.sa_last_error(ch._h)
        assert fn(ch._h, None, out.data_ptr(), B, kind, stream) == SA_EINVAL
        assert fn(ch._h, d.data_ptr(), None, B, kind, stream) == SA_EINVAL
        assert fn(ch._h, d.data_ptr(), out.data_ptr(), A + 1, kind, stream) == SA_ESHAPE
        assert fn(ch._h, None, None, A + 1, kind, stream) == SA_ESHAPE                  # the batch before the pointers
        assert fn(ch._h, None, None, 0, kind, stream) == 0
    xf = torch.zeros((B, N), dtype=torch.float32, device="cuda")
    of = torch.full((B, N), 3.0, dtype=torch.float32, device="cuda")
    assert L.sa_process_f32(ch._h, xf.data_ptr(), of.data_ptr(), B, kind, stream) == SA_EINVAL
    assert L.sa_process_f32_i16(ch._h, xd.data_ptr(), 1.0, of.data_ptr(), B, kind, stream) == SA_EINVAL
    assert L.sa_process_f32_p12(ch._h, pd.data_ptr(), 1.0, of.data_ptr(), B, kind, stream) == SA_EINVAL
    assert untouched(True) and (of == 3.0).all().item()
    assert len(ch.profile_read(64)) == timed        # no refused call was timed: no call state committed
    ch.set_profiling(0)
    for fn, d in calls:
        assert fn(ch._h, d.data_ptr(), out.data_ptr(), B, kind, stream) == 0
        _check(out, mag, ip, W, A, "after refusals")
        assert untouched(False)
        bigt.fill_(canary)
    for bad in (0, 1, 3, 256, 2.0, True):
        with pytest.raises(SpecanError) as e:
            ch.traces_q15(xd[:B], bucket=W, group=bad)
        assert e.value.code == SA_EINVAL, bad
    with pytest.raises(SpecanError) as e:
        ch.traces_q15(xd[:6], bucket=W, group=4)
    assert e.value.code == SA_ESHAPE
    with pytest.raises(SpecanError) as e:
        ch.traces_q15(xd[:B], bucket=W, group=A, out=torch.empty((B, N // W, 2), dtype=torch.float32, device="cuda"))
    assert e.value.code == SA_ESHAPE
    _check(ch.traces_q15(xd[:B], bucket=W, group=A), mag, ip, W, A, "after wrapper refusals")
    e0 = torch.empty((0, N), dtype=torch.int16, device="cuda")
    assert ch.traces_q15(e0, bucket=64, group=128).shape == (0, N // 64, 2)
    assert torch.equal(ch.traces_q15(xd[:B], bucket=W, group=None), ch.traces_q15(xd[:B], bucket=W))
