"""GPU: the integer chain on packed 12-bit samples (sa_process_q15_p12, sa_filter_q15_p12; the format is defined in
include/specan.h).

The criterion throughout is torch.equal against the int16 call on the same samples: the packed entry points unpack inside
the kernels that read the samples and then ARE the int16 path, so there are no tolerances.  One test goes past the int16
kernels' loads and compares with the integer model on ingest.unpack12 of the packed bytes."""
import functools

import numpy as np
import pytest

from conftest import N
from gpu_support import ch, check_overlap_profiling_and_graph_capture, to_device, torch_mod  # noqa: F401 (fixtures)
from fpga_real_time_fft_analyzer_amd.abi import SA_P12_FRAME_BYTES as P12
from q15_cases import call, configure

pytestmark = pytest.mark.gpu

KINDS = ("iq", "mag", "marker")
SEAMS = (2, 5, 1026,            # the straddling lanes of FFT stage 0
         7, 8,                  # a lane's 8-sample unit
         255, 256,              # a tile
         511, 512,              # the ring wrap
         1023, 1024,            # the stage-0 stride
         8191, 8192, 16376, 16382, 16383)
MODES = ("0xB1", "0x00", "0xA1-b1", "0xA1-zero-b1", "0xA2-six", "0xA2-none")           # of q15_cases.SETUPS


@functools.lru_cache(maxsize=None)
def batch():
    """(int16 [17,N], packed uint8 [17,24576]) of the same samples, read-only.  Rows 0..4 are the batch of most tests:
    0 random in [-2048, 2047]; 1 the alternating extremes; 2 the ramp (37 n mod 4096) - 2048, on which a misplaced sample
    shows; 3 zero; 4 zero except single samples at SEAMS.  Rows 5..16 are random: with them a cascade launch has a second
    workgroup that holds one frame (a workgroup holds 16, a wave 4)."""
    from fpga_real_time_fft_analyzer_amd.ingest import pack12
    rng = np.random.default_rng(1210)
    n = np.arange(N)
    x = rng.integers(-2048, 2048, (17, N)).astype(np.int16)
    x[1] = np.where(n & 1, 2047, -2048)
    x[2] = (37 * n) % 4096 - 2048
    x[3] = 0
    x[4] = 0
    for k, pos in enumerate(SEAMS):
        x[4, pos] = (-1) ** k * (100 + 120 * k)
    p = pack12(x)
    assert p.shape == (17, P12) and p.dtype == np.uint8
    x.setflags(write=False)
    p.setflags(write=False)
    return x, p


def assert_packed_equals_int16(torch, ch, d_p, d_i, what):
    for kind in KINDS + ("filter",):
        a, b = call(ch, kind, d_p), call(ch, kind, d_i)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (what, kind)
        assert b.any(), (what, kind)                               # the comparison is not between two empty results


@pytest.mark.parametrize("win_mode", [0, 1])
@pytest.mark.parametrize("mode", MODES)
def test_packed_equals_int16_for_every_mode_and_kind(ch, torch_mod, mode, win_mode):
    x, p = batch()
    d_i, d_p = to_device(torch_mod, x[:5]), to_device(torch_mod, p[:5])
    configure(ch, mode)
    ch.set_window_mode_q15(win_mode)
    assert_packed_equals_int16(torch_mod, ch, d_p, d_i, (mode, win_mode))


def test_packed_equals_int16_with_a_custom_rom(ch, torch_mod):
    x, p = batch()
    d_i, d_p = to_device(torch_mod, x[:5]), to_device(torch_mod, p[:5])
    ch.set_window_q15(np.random.default_rng(3).integers(-32768, 32768, N).astype(np.int16))
    for mode in ("0xB1", "0x00", "0xA2-six"):
        configure(ch, mode)
        assert_packed_equals_int16(torch_mod, ch, d_p, d_i, mode)


@pytest.mark.parametrize("mode", ["0xB1", "0x00", "0xA2-six"])
def test_sample_order_against_the_integer_model(ch, torch_mod, oracle, mode):
    """An order check that does not go through the int16 kernels' loads: the integer model on unpack12 of the bytes."""
    from fpga_real_time_fft_analyzer_amd.ingest import unpack12
    x, p = batch()
    d_p = to_device(torch_mod, p[:5])
    _, _, cmd, c12, sos = configure(ch, mode)
    s = unpack12(p[:5])
    assert np.array_equal(s, x[:5])
    ref_iq, ref_t = oracle.chain_q15(s, None, 0, cmd, c12, sos, want_time=True)
    assert np.array_equal(ch.filter_q15(d_p).cpu().numpy(), ref_t)
    assert np.array_equal(ch.process_q15(d_p).cpu().numpy(), ref_iq) and ref_iq.any()


@pytest.mark.parametrize("mode", ["0xB1", "0x00", "0xA2-six"])
def test_batch_geometry(ch, torch_mod, mode):
    """B = 1, 5 and 17 give the rows of the int16 call; each frame alone equals its row of the batch call; a whole-frame
    slice of a larger tensor (its data pointer is offset by whole frames) equals the matching rows."""
    torch = torch_mod
    x, p = batch()
    d_i, d_p = to_device(torch, x), to_device(torch, p)
    configure(ch, mode)
    for kind in ("iq", "marker", "filter"):
        ref = call(ch, kind, d_i).clone()
        for B in (1, 5, 17):
            assert torch.equal(call(ch, kind, d_p[:B]), ref[:B]), (kind, B)
        for f in (0, 4, 16):
            assert torch.equal(call(ch, kind, d_p[f:f + 1].clone()), ref[f:f + 1]), (kind, f)
        big = torch.full((7, P12), 0x5A, dtype=torch.uint8, device="cuda")
        big[2:5] = d_p[1:4]
        part = big[2:5]
        assert part.is_contiguous() and part.data_ptr() == big.data_ptr() + 2 * P12
        assert torch.equal(call(ch, kind, part), ref[1:4]), kind


def test_marker_range_that_cuts_the_spectrum(ch, torch_mod):
    torch = torch_mod
    x, p = batch()
    d_i, d_p = to_device(torch, x[:5]), to_device(torch, p[:5])
    ch.set_marker_range(100, 5000)
    for mode in ("0xB1", "0x00"):
        configure(ch, mode)
        rec_p, rec_i = ch.process_q15(d_p, out_kind="marker"), ch.process_q15(d_i, out_kind="marker")
        assert torch.equal(rec_p, rec_i) and rec_i.any(), mode
        _, peak_bin, _ = ch.markers_q15(d_p)
        assert ((peak_bin >= 100) & (peak_bin < 5000)).all()


@pytest.mark.parametrize("mode", ["0x00", "0xA2-six"])
def test_overlap_profiling_and_graph_capture(ch, torch_mod, mode):
    """Everything that holds for the int16 entry point's launches: overlap depth 2 with flush (in 0xA2 the wide cascade's
    ordering behind the previous call), one device time per timed call, and capture into a graph after reserve; all
    outputs equal the plain stream-ordered int16 call."""
    torch = torch_mod
    x, p = batch()
    d_i, d_p = to_device(torch, x[:5]), to_device(torch, p[:5])
    configure(ch, mode)
    ch.reserve(8)
    ref = ch.process_q15(d_i).clone()
    assert ref.any()
    check_overlap_profiling_and_graph_capture(torch, ch, lambda out: ch.process_q15(d_p, out=out), ref)


def test_argument_errors(ch, torch_mod):
    from fpga_real_time_fft_analyzer_amd.abi import SA_EINVAL, SA_ESHAPE, SA_OK, SA_Q15_OUT_IQ, SA_Q15_OUT_MARKER, SpecanError
    torch = torch_mod
    x, p = batch()
    d_i, d_p = to_device(torch, x[:2]), to_device(torch, p[:2])
    ch.set_filter_mode(0x00)
    ref = ch.process_q15(d_i).clone()
    ref_t = ch.filter_q15(d_i).clone()
    flat = torch.zeros(8 + 2 * P12, dtype=torch.uint8, device="cuda")
    off = flat[8:].view(2, P12)                                    # contiguous, 8 bytes off a 16-byte boundary
    off.copy_(d_p)
    assert off.is_contiguous() and off.data_ptr() % 16 == 8
    for fn in (ch.process_q15, ch.filter_q15):
        with pytest.raises(SpecanError) as e:
            fn(off)
        assert e.value.code == SA_EINVAL
    assert torch.equal(ch.process_q15(d_p), ref)                   # nothing was launched, no call state changed
    assert torch.equal(ch.filter_q15(d_p), ref_t)
    for fn in (ch.process_q15, ch.filter_q15):
        with pytest.raises(SpecanError) as e:
            fn(torch.zeros((2, P12 - 1), dtype=torch.uint8, device="cuda"))
        assert e.value.code == SA_ESHAPE
    with pytest.raises(SpecanError) as e:
        ch.process_q15(d_p, out_kind="mag_full")                   # a kind of the float path
    assert e.value.code == SA_EINVAL
    # the C entry point's own checks
    L, h, s = ch._lib, ch._h, ch._stream()
    out = torch.zeros((2, N, 2), dtype=torch.int16, device="cuda")
    rec = torch.zeros(8 + 2 * 16, dtype=torch.uint8, device="cuda")
    assert L.sa_process_q15_p12(h, d_p.data_ptr(), out.data_ptr(), 2, 7, s) == SA_EINVAL               # unknown kind
    assert L.sa_process_q15_p12(h, d_p.data_ptr(), out.data_ptr(), 2, -1, s) == SA_EINVAL
    assert L.sa_process_q15_p12(h, d_p.data_ptr(), rec.data_ptr() + 8, 2, SA_Q15_OUT_MARKER, s) == SA_EINVAL
    assert L.sa_process_q15_p12(h, None, out.data_ptr(), 2, SA_Q15_OUT_IQ, s) == SA_EINVAL
    assert L.sa_process_q15_p12(h, d_p.data_ptr(), None, 2, SA_Q15_OUT_IQ, s) == SA_EINVAL
    assert L.sa_process_q15_p12(h, d_p.data_ptr(), out.data_ptr(), -1, SA_Q15_OUT_IQ, s) == SA_ESHAPE
    assert L.sa_filter_q15_p12(h, d_p.data_ptr() + 8, out.data_ptr(), 2, s) == SA_EINVAL
    torch.cuda.synchronize()
    assert not out.any() and not rec.any()                         # nothing was launched
    assert L.sa_process_q15_p12(h, d_p.data_ptr(), out.data_ptr(), 2, SA_Q15_OUT_IQ, s) == SA_OK
    assert torch.equal(out, ref)


def test_packed_feeder_gives_the_int16_feeders_frames(ch, torch_mod):
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
    ch.set_filter_mode(0x00)

    def run(feeder, frames):
        got = [ch.process_q15(xd).clone() for xd in feeder.feed(frames[i:i + 8] for i in range(0, len(frames), 8))]
        torch.cuda.synchronize()
        return torch.cat(got)

    out_i = run(DeviceFeeder(0, max_batch=8), frames_i)
    out_p = run(DeviceFeeder(0, max_batch=8, packed=True), frames_p)
    assert out_p.shape == (19, N, 2) and torch.equal(out_p, out_i) and out_i.any()


def test_virtual_fpga_with_a_packed_source(torch_mod):
    from fpga_real_time_fft_analyzer_amd.virtual_fpga import VirtualFpga
    x, p = batch()

    def frames_of(src):
        served = []

        def source(n):
            i = len(served)
            served.extend(range(i, i + n))
            return src[[j % 5 for j in range(i, i + n)]]

        fpga = VirtualFpga(source, device=0, batch=3)
        try:
            fpga.write(bytes([0x00, 0x55]))                        # default cascade, Ethernet streaming
            dg = fpga.read_datagrams(7)
            assert len(served) == 9
            return b"".join(d[1:] for d in dg)
        finally:
            fpga.close()

    got_i, got_p = frames_of(x), frames_of(p)
    assert len(got_i) == 7 * 65536 and got_p == got_i and any(got_i)
