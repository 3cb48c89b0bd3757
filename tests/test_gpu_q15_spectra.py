"""GPU: full-resolution max hold and summed power over groups of A = 2^a frames (include/specan_ext.h: sa_spectra_q15,
sa_spectra_q15_p12, sa_fold_iq_q15 -- one {peak_mag, power} record per bin and group), through SpectrumChain.spectra_q15 and
SpectrumChain.fold_iq_q15 and the three C entry points.

Every comparison is exact, on float bits.  The reference of the chain calls is the call they derive from: the handle's own
process_q15(..., out_kind="iq") on the same input, reduced in numpy in int64 -- the peak is the maximum over the group of
frames.decode_mag_16iq_le, the power the int64 sum of re^2 + im^2 over the group converted once to float32 (nearest even;
tests/test_q15_trace_avg_cpu.py pins that conversion up to 2^44).  The first test holds those frames to the oracle's too.  The
reference of the fold alone is the numpy mirror frames.spectrum_of_frames."""
import numpy as np
import pytest

from conftest import N
from gpu_support import ch, check_overlap_profiling_and_graph_capture, to_device, torch_mod  # noqa: F401 (fixtures)
from fpga_real_time_fft_analyzer_amd.abi import SA_EINVAL, SA_ESHAPE, SA_ESTATE
from q15_cases import SETUP_OF_MODE, SETUPS, configure, handle_iq as _iq, records_equal, uniform
from q15_mirrors import bits as _bits, decode as _decode, spectra_expect as _expect

pytestmark = pytest.mark.gpu

FORMS = ("b1_rtl", "b1_rom_hann_u16", "default", "gui_upload", "wide6")       # of q15_cases.SETUPS
SHAPES = ((2, 2), (2, 6), (4, 8), (8, 24))                   # (A, B): every B is a prefix of one 24-frame batch


def _check(rec, mag, ip, A, tag=""):
    """a [B/A,N,2] float32 record tensor against numpy on the decoded frames, by bits"""
    peak, power, _ = _expect(mag, ip, A)
    records_equal(rec, peak, power, (mag.shape[0] // A, N, 2), (tag, A))


@pytest.mark.parametrize("form", FORMS)
def test_records_equal_numpy(ch, torch_mod, oracle, form):
    """Modes 0xB1 (RTL window; a custom ROM in the 16-bit Hann mode), 0x00, 0xA1 with the GUI upload and 0xA2 with six
    sections; (A, B) = (2,2), (2,6), (4,8), (8,24) -- the first B frames of one 24-frame batch whose frames 2 and 3 are zero, so
    that in (2,6) group 1 is all zero: its records have all bits zero, and its neighbours' do not; 12-bit samples as int16 and
    packed, and full-scale int16.  In 0xB1 also (128,128) and (128,256).  The handle's IQ frames, the reference, are the
    oracle's for the 24-frame batches; the chain call equals the fold alone on those frames, and (0xB1, RTL) the largest peak of
    each bucket of 16 records is the grouped trace's peak of that bucket."""
    from fpga_real_time_fft_analyzer_amd.ingest import pack12
    torch = torch_mod
    rng = np.random.default_rng(1400 + FORMS.index(form))
    args = configure(ch, form, rng)
    for full in (False, True):
        x = uniform(rng, (24, N), full)
        x[2:4] = 0
        xd = to_device(torch, x)
        pd = None if full else to_device(torch, pack12(x))
        iqd = ch.process_q15(xd, out_kind="iq")
        ref = iqd.cpu().numpy()
        assert np.array_equal(ref, oracle.chain_q15(x, *args)), (form, full)
        mag, ip = _decode(ref)
        assert mag[:2].any() and not ref[2:4].any()
        for A, B in SHAPES:
            tag = (form, full, A, B)
            rec = ch.spectra_q15(xd[:B], A)
            _check(rec, mag[:B], ip[:B], A, tag + ("int16",))
            if pd is not None:
                _check(ch.spectra_q15(pd[:B], A), mag[:B], ip[:B], A, tag + ("p12",))
            assert torch.equal(ch.fold_iq_q15(iqd[:B], A).view(torch.int32), rec.view(torch.int32)), tag
            if (A, B) == (2, 6):
                assert not rec[1].view(torch.int32).any().item(), tag
                assert rec[0].view(torch.int32).any().item() and rec[2].view(torch.int32).any().item(), tag
            if form == "b1_rtl" and (A, B) == (4, 8):
                avg = ch.traces_q15(xd[:B], bucket=16, group=A)
                top = rec[..., 0].contiguous().view(B // A, N // 16, 16).amax(2)
                assert torch.equal(top.contiguous().view(torch.int32), avg[..., 0].contiguous().view(torch.int32)), tag
    if SETUPS[form].cmd != 0xB1:
        return
    for full in (False, True):
        x = uniform(rng, (256, N), full)
        xd = to_device(torch, x)
        pd = None if full else to_device(torch, pack12(x))
        mag, ip = _decode(_iq(ch, xd))
        for B in (128, 256):
            _check(ch.spectra_q15(xd[:B], 128), mag[:B], ip[:B], 128, (form, full, B, "int16"))
            if pd is not None:
                _check(ch.spectra_q15(pd[:B], 128), mag[:B], ip[:B], 128, (form, full, B, "p12"))


@pytest.mark.parametrize("A,B", [(2, 2), (4, 8), (128, 256)])
def test_fold_alone_against_the_mirror(ch, torch_mod, A, B):
    """IQ that no chain produces: random full-scale int16 with a block of 64 bins at (-32768, -32768), 2^31 each, and an all-zero
    frame in group 0.  The last group keeps the block in all of its A frames: A 2^31 per bin, 2^38 at A = 128, the largest sum
    there is.  By bits against frames.spectrum_of_frames, group by group."""
    from fpga_real_time_fft_analyzer_amd import frames
    torch = torch_mod
    rng = np.random.default_rng(1500 + A)
    iq = rng.integers(-32768, 32768, size=(B, N, 2)).astype(np.int16)
    iq[:, 100:164] = -32768
    iq[A // 2] = 0
    rec = ch.fold_iq_q15(to_device(torch, iq), A)
    assert tuple(rec.shape) == (B // A, N, 2) and rec.dtype == torch.float32
    r = rec.cpu().numpy()
    le = iq.astype("<i2", copy=False)
    for g in range(B // A):
        peak, power, exact = frames.spectrum_of_frames([le[f].tobytes() for f in range(g * A, (g + 1) * A)])
        want = (A - (g == 0)) << 31
        assert (exact[100:164] == want).all() and exact.max() == want, (A, B, g)
        bad = np.nonzero(_bits(r[g, :, 0]) != _bits(peak))[0]
        assert bad.size == 0, (A, B, g, "peak", bad[:5], r[g, bad[:5], 0], peak[bad[:5]])
        bad = np.nonzero(_bits(r[g, :, 1]) != _bits(power))[0]
        assert bad.size == 0, (A, B, g, "power", bad[:5], r[g, bad[:5], 1], power[bad[:5]])
    if A == 128:
        assert want == 1 << 38 and B // A == 2
    z = ch.fold_iq_q15(torch.zeros((A, N, 2), dtype=torch.int16, device="cuda"), A)
    assert not z.view(torch.int32).any().item()                                      # (+0, +0) everywhere


def test_offsets_past_4_gib(ch, torch_mod):
    """fold_iq_q15 at A = 2 on 65536 + 2 frames generated on the device, 4 GiB + 128 KiB of input: the last row reads from byte
    2^32 on.  It equals the fold of the last two frames alone, and so do rows 0 and 20000, compared on the device."""
    torch = torch_mod
    B = 65536 + 2
    gen = torch.Generator(device="cuda")
    gen.manual_seed(99)
    tile = torch.randint(-32768, 32768, (1027, N, 2), dtype=torch.int16, device="cuda", generator=gen)
    iq = torch.empty((B, N, 2), dtype=torch.int16, device="cuda")
    for f in range(0, B, 1027):                                                      # period 1027 frames: no two rows read alike
        n = min(1027, B - f)
        iq[f:f + n] = tile[:n]
    iq[-2:] = torch.randint(-32768, 32768, (2, N, 2), dtype=torch.int16, device="cuda", generator=gen)
    assert iq[-2:].data_ptr() - iq.data_ptr() == 1 << 32
    rec = ch.fold_iq_q15(iq, 2)
    assert tuple(rec.shape) == (B // 2, N, 2)
    for row in (B // 2 - 1, 0, 20000):
        alone = ch.fold_iq_q15(iq[2 * row:2 * row + 2], 2)
        assert alone.view(torch.int32).any().item(), row
        assert torch.equal(rec[row].view(torch.int32), alone[0].view(torch.int32)), row
    assert not torch.equal(rec[-1], rec[0])
    del rec, iq, tile
    torch.cuda.empty_cache()


@pytest.mark.parametrize("hop", [8, 4096, 16376, 16384])
def test_hop_streams(ch, torch_mod, hop):
    """One sample stream, int16 and packed, cut on the device: B = 8, A = 4 equals the frame call on the frames cut on the
    host, in mode 0xB1 (the FFT reads the stream) and 0x00 (the cascade does), and both equal the reference."""
    from fpga_real_time_fft_analyzer_amd.ingest import pack12
    torch = torch_mod
    rng = np.random.default_rng(hop)
    A, B = 4, 8
    for cmd in (0xB1, 0x00):
        ch.set_filter_mode(cmd)
        s = rng.integers(-2048, 2048, size=(B - 1) * hop + N).astype(np.int16)
        fr = np.stack([s[i * hop:i * hop + N] for i in range(B)])
        sd, fd = to_device(torch, s), to_device(torch, fr)
        sp, fp = to_device(torch, pack12(s)), to_device(torch, pack12(fr))
        mag, ip = _decode(_iq(ch, fd))
        want = ch.spectra_q15(fd, A)
        _check(want, mag, ip, A, (hop, hex(cmd)))
        assert torch.equal(ch.spectra_q15(sd, A, hop=hop), want), (hop, hex(cmd))
        assert torch.equal(ch.spectra_q15(sp, A, hop=hop), want), (hop, hex(cmd), "p12")
        assert torch.equal(ch.spectra_q15(fp, A), want), (hop, hex(cmd), "p12 frames")


@pytest.mark.parametrize("cmd", [0xB1, 0x00, 0xA2])
def test_overlap_profiling_and_graph_capture(ch, torch_mod, cmd):
    """The call in the unstaged launch (0xB1: FFT, fold) and the staged one (0x00, 0xA2 with six sections: cascade, FFT, fold),
    and the fold alone: overlap depth 2 with flush equals the ordered result, one device time per timed call, capture into a
    graph.  The reference call is the warm-up that grows slot 0's workspaces.  Then an `out` one row longer than needed,
    filled with a canary, keeps its last row."""
    torch = torch_mod
    rng = np.random.default_rng(69)
    x = rng.integers(-2048, 2048, size=(8, N)).astype(np.int16)
    configure(ch, SETUP_OF_MODE[cmd])
    xd = to_device(torch, x)
    iqd = ch.process_q15(xd, out_kind="iq")
    mag, ip = _decode(iqd.cpu().numpy())
    for A in (4, 2):
        ref = ch.spectra_q15(xd, A).clone()
        _check(ref, mag, ip, A, hex(cmd))
        for _ in range(3):
            assert torch.equal(ch.spectra_q15(xd, A), ref), (hex(cmd), A)
        check_overlap_profiling_and_graph_capture(torch, ch, lambda o: ch.spectra_q15(xd, A, out=o), ref)
        check_overlap_profiling_and_graph_capture(torch, ch, lambda o: ch.fold_iq_q15(iqd, A, out=o), ref)
    canary = 0x7FC0BEEF
    big = torch.full((3, N, 2), canary, dtype=torch.int32, device="cuda")
    ch.spectra_q15(xd, 4, out=big[:2].view(torch.float32))
    torch.cuda.synchronize()
    assert torch.equal(big[:2], ch.spectra_q15(xd, 4).view(torch.int32)) and (big[2] == canary).all().item()
    big.fill_(canary)
    ch.fold_iq_q15(iqd, 4, out=big[:2].view(torch.float32))
    torch.cuda.synchronize()
    assert torch.equal(big[:2], ch.spectra_q15(xd, 4).view(torch.int32)) and (big[2] == canary).all().item()


@pytest.mark.parametrize("cmd", [0xB1, 0x00])
def test_capture_needs_one_call_of_that_batch_first(ch, torch_mod, cmd):
    """A fresh handle (after reserve, which sizes nothing for this call): inside a capture the fold alone is taken, and the
    chain call is SA_ESTATE with a message that names the remedy and nothing of it launched -- the graph replays the fold
    alone.  After one call of that batch outside the capture it captures and replays; a larger batch is refused again."""
    from fpga_real_time_fft_analyzer_amd.abi import SpecanError
    torch = torch_mod
    rng = np.random.default_rng(70)
    x = rng.integers(-2048, 2048, size=(16, N)).astype(np.int16)
    xd = to_device(torch, x)
    ch.set_filter_mode(cmd)
    ch.reserve(16)
    iqd = ch.process_q15(xd, out_kind="iq")
    mag, ip = _decode(iqd.cpu().numpy())
    out = torch.zeros((2, N, 2), dtype=torch.float32, device="cuda")
    held = torch.full((2, N, 2), 7.0, dtype=torch.float32, device="cuda")
    graph = torch.cuda.CUDAGraph()
    refused = []
    with torch.cuda.graph(graph):
        ch.fold_iq_q15(iqd[:8], 4, out=out)
        try:
            ch.spectra_q15(xd[:8], 4, out=held)
            refused.append("accepted")
        except SpecanError as e:
            refused.append((e.code, "outside the capture" in str(e), "sa_spectra_q15" in str(e)))
    assert refused == [(SA_ESTATE, True, True)], refused
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    _check(out, mag[:8], ip[:8], 4, "captured fold")
    assert (held == 7.0).all().item()                                                # the refused call wrote nothing
    _check(ch.spectra_q15(xd[:8], 4, out=held), mag[:8], ip[:8], 4, "outside the capture")   # grows the workspace
    graph2 = torch.cuda.CUDAGraph()
    big = torch.full((4, N, 2), 7.0, dtype=torch.float32, device="cuda")
    refused = []
    with torch.cuda.graph(graph2):
        ch.spectra_q15(xd[:8], 4, out=held)
        try:
            ch.spectra_q15(xd, 4, out=big)                                           # 16 frames: the workspace holds 8
            refused.append("accepted")
        except SpecanError as e:
            refused.append(e.code)
    assert refused == [SA_ESTATE]
    held.zero_()
    graph2.replay()
    torch.cuda.synchronize()
    _check(held, mag[:8], ip[:8], 4, "captured after one call")
    assert (big == 7.0).all().item()
    _check(ch.spectra_q15(xd, 4, out=big), mag, ip, 4, "after the captures")


def test_refusals_leave_the_handle_usable(ch, torch_mod):
    """Through Python: a bad group (SA_EINVAL), B no multiple of it (SA_ESHAPE), an `out` 8 bytes off and an `out` that meets the
    input (SA_EINVAL, from the C entry point, with the contract's message), a wrong shape or dtype.  Through the C entry
    points: log2a and hop out of range, also at batch 0, NULL, the batch before the pointers.  No refused call shows in the
    profiling ring or changes a byte of `out`, and a good call afterwards is correct."""
    from fpga_real_time_fft_analyzer_amd import abi
    from fpga_real_time_fft_analyzer_amd.abi import SpecanError
    from fpga_real_time_fft_analyzer_amd.ingest import pack12
    torch = torch_mod
    rng = np.random.default_rng(15)
    A, B = 4, 8
    x = rng.integers(-2048, 2048, size=(B + 1, N)).astype(np.int16)
    ch.set_filter_mode(0x00)
    xd, pd = to_device(torch, x), to_device(torch, pack12(x))
    iqd = ch.process_q15(xd[:B], out_kind="iq")
    mag, ip = _decode(iqd.cpu().numpy())
    ch.set_profiling(16)
    ref = ch.spectra_q15(xd[:B], A).clone()
    _check(ref, mag, ip, A, "good call")
    assert len(ch.profile_read(16)) == 1

    def refused(code, call, *a, **k):
        with pytest.raises(SpecanError) as e:
            call(*a, **k)
        assert e.value.code == code, (a, k, str(e.value))
        return str(e.value)

    for bad in (0, 1, 3, 256, 2.0, True, None):
        refused(SA_EINVAL, ch.spectra_q15, xd[:B], bad)
        refused(SA_EINVAL, ch.fold_iq_q15, iqd, bad)
    refused(SA_ESHAPE, ch.spectra_q15, xd[:6], 4)
    refused(SA_ESHAPE, ch.spectra_q15, xd, 2)                                        # 9 frames
    refused(SA_ESHAPE, ch.fold_iq_q15, iqd[:6], 4)
    refused(SA_ESHAPE, ch.spectra_q15, xd[:B], A, out=torch.empty((B, N, 2), dtype=torch.float32, device="cuda"))
    refused(SA_ESHAPE, ch.spectra_q15, xd[:B], A, out=torch.empty((B // A, N, 2), dtype=torch.int32, device="cuda"))
    refused(SA_ESHAPE, ch.fold_iq_q15, iqd.view(B, 2 * N), A)
    refused(SA_EINVAL, ch.fold_iq_q15, iqd.view(torch.float32), A)
    refused(SA_EINVAL, ch.spectra_q15, xd[:B].float(), A)
    for hop in (4, 12, 16392, 8.0, True):
        refused(SA_EINVAL, ch.spectra_q15, xd[:B].reshape(-1), A, hop=hop)
    # an `out` 8 bytes off
    canary = 7.0
    n = (B // A) * N * 2
    flat = torch.full((n + 4,), canary, dtype=torch.float32, device="cuda")
    off8 = flat[2:2 + n].view(B // A, N, 2)
    assert off8.data_ptr() % 16 == 8
    assert "16-byte aligned" in refused(SA_EINVAL, ch.spectra_q15, xd[:B], A, out=off8)
    assert "16-byte aligned" in refused(SA_EINVAL, ch.fold_iq_q15, iqd, A, out=off8)
    # an `out` whose first 16 bytes are the input's last: one buffer, the input in front
    for make_in, call, n_in in ((lambda b: b.view(torch.int16).view(B, N), ch.spectra_q15, B * N * 2),
                                (lambda b: b.view(torch.int16).view(B, N, 2), ch.fold_iq_q15, B * N * 4)):
        buf = torch.zeros((n_in + 4 * n,), dtype=torch.uint8, device="cuda")
        src = make_in(buf[:n_in])
        src.copy_(xd[:B] if call == ch.spectra_q15 else iqd)
        meets = buf[n_in - 16:n_in - 16 + 4 * n].view(torch.float32).view(B // A, N, 2)
        msg = refused(SA_EINVAL, call, src, A, out=meets)
        assert f"({n_in} bytes read)" in msg and f"({4 * n} bytes written) overlap" in msg, msg
        assert torch.equal(src, xd[:B] if call == ch.spectra_q15 else iqd)
        touches = buf[n_in:n_in + 4 * n].view(torch.float32).view(B // A, N, 2)      # right behind it: fine
        assert torch.equal(call(src, A, out=touches), ref)
    timed = len(ch.profile_read(16))
    assert timed == 3                                                                # the good call and the two that touch
    # the C entry points
    L = abi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.full((B // A, N, 2), canary, dtype=torch.float32, device="cuda")
    for fn, d in ((L.sa_spectra_q15, xd), (L.sa_spectra_q15_p12, pd)):
        for batch in (B, 0):
            for a in (0, 8, -1):
                assert fn(ch._h, d.data_ptr(), out.data_ptr(), batch, a, 0, stream) == SA_EINVAL, (a, batch)
            for hop in (4, 12, 16392, -8):
                assert fn(ch._h, d.data_ptr(), out.data_ptr(), batch, 2, hop, stream) == SA_EINVAL, (hop, batch)
        assert fn(ch._h, d.data_ptr(), out.data_ptr(), -1, 0, 4, stream) == SA_ESHAPE    # the batch before the arguments
        assert fn(ch._h, None, None, B + 1, 2, 0, stream) == SA_ESHAPE                   # the group before the pointers
        assert fn(ch._h, None, out.data_ptr(), B, 2, 0, stream) == SA_EINVAL
        assert fn(ch._h, d.data_ptr(), None, B, 2, 0, stream) == SA_EINVAL
        assert fn(ch._h, d.data_ptr(), out.data_ptr() + 8, B, 2, 0, stream) == SA_EINVAL
        assert fn(ch._h, None, None, 0, 2, 0, stream) == 0
        assert fn(None, d.data_ptr(), out.data_ptr(), B, 2, 0, stream) == SA_EINVAL
    for batch in (B, 0):
        assert L.sa_fold_iq_q15(ch._h, iqd.data_ptr(), out.data_ptr(), batch, 0, stream) == SA_EINVAL
    assert L.sa_fold_iq_q15(ch._h, None, None, B + 1, 2, stream) == SA_ESHAPE
    assert L.sa_fold_iq_q15(ch._h, iqd.data_ptr(), None, B, 2, stream) == SA_EINVAL
    assert L.sa_fold_iq_q15(ch._h, None, None, 0, 2, stream) == 0
    torch.cuda.synchronize()
    assert (out == canary).all().item() and (flat == canary).all().item()
    assert len(ch.profile_read(16)) == timed                                         # no refused call was timed
    ch.set_profiling(0)
    # the handle goes on
    for fn, d in ((L.sa_spectra_q15, xd), (L.sa_spectra_q15_p12, pd)):
        out.fill_(canary)
        assert fn(ch._h, d.data_ptr(), out.data_ptr(), B, 2, 0, stream) == 0
        assert torch.equal(out, ref)
    assert torch.equal(ch.fold_iq_q15(iqd, A), ref)
    e0 = torch.empty((0, N), dtype=torch.int16, device="cuda")
    assert ch.spectra_q15(e0, 128).shape == (0, N, 2)
    assert ch.fold_iq_q15(torch.empty((0, N, 2), dtype=torch.int16, device="cuda"), 2).shape == (0, N, 2)
