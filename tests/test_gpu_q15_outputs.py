"""GPU: the SA_Q15_OUT_MAG and SA_Q15_OUT_MARKER outputs of the integer chain (include/specan.h, sa_process_q15_out),
through the C ABI via SpectrumChain.process_q15(out_kind=...) / markers_q15.

Every comparison is exact (np.array_equal on float bits and integers): the outputs are bit-defined.  The expected values
come from frames.decode_mag_16iq_le (the committed mirror of gui.py:250-260, pinned by tests/golden/g6_frame.npz) and
frames.marker_of_frame's arithmetic (slice, max / argmax, int64 sum of squares) applied to (a) the ORACLE's frame
oracle.chain_q15(...) and (b) the handle's own process_q15 IQ output, asserted equal to (a) first.
"""
import numpy as np
import pytest

from conftest import N
from gpu_support import ch, to_device, torch_mod  # noqa: F401 (fixtures)
from fpga_real_time_fft_analyzer_amd.abi import SA_EINVAL, SA_ESHAPE
from q15_cases import configure, extreme_frames, uniform, wide_sections
from q15_mirrors import bits as _bits, decode as _decode, marker_expect as _expect, marker_records as _records

pytestmark = pytest.mark.gpu

# RANGES of tests/test_gpu_marker.py, plus the two the Q15 contract adds
RANGES = [(0, N), (0, 8193), (100, 2000), (9000, 12000), (8000, 8400), (0, 1), (8192, 8193), (16383, 16384),
          (8193, N), (5, 6)]


def _check_marker(rec, mag, ip, lo, hi, tag=""):
    pm, pb, bp = _records(rec)
    wm, wb, wp = _expect(mag, ip, lo, hi)
    assert np.array_equal(_bits(pm), _bits(wm)), (tag, lo, hi, np.nonzero(_bits(pm) != _bits(wm))[0][:5])
    assert np.array_equal(pb, wb), (tag, lo, hi, pb[pb != wb][:5], wb[pb != wb][:5])
    assert np.array_equal(bp, wp), (tag, lo, hi, bp[bp != wp][:5], wp[bp != wp][:5])


def _check_all(ch, torch_mod, xd, ref_iq, ranges=RANGES, tag=""):
    """IQ == oracle, MAG == decode of it, MARKER == numpy on that decode for every range; returns (mag, ip)"""
    torch = torch_mod
    B = ref_iq.shape[0]
    iq = ch.process_q15(xd).cpu().numpy()
    assert np.array_equal(iq, ref_iq), tag                       # side (b) is side (a)
    mag, ip = _decode(ref_iq)
    got = ch.process_q15(xd, out_kind="mag")
    assert got.shape == (B, N) and got.dtype == torch.float32
    got = got.cpu().numpy()
    bad = np.nonzero(_bits(got) != _bits(mag))
    assert bad[0].size == 0, (tag, "MAG differs", bad[0][:5], bad[1][:5], got[bad][:5], mag[bad][:5])
    for lo, hi in ranges:
        ch.set_marker_range(lo, hi)
        rec = ch.process_q15(xd, out_kind="marker")
        assert rec.shape == (B, 4) and rec.dtype == torch.int32
        _check_marker(rec, mag, ip, lo, hi, tag)
    return mag, ip


def _samples(rng, B, full_scale):
    """12-bit or full-scale random samples; from B = 7 on: frame 1 all zero, the last frame of the other scale"""
    x = uniform(rng, (B, N), full_scale)
    if B >= 7:
        x[1] = 0
        x[-1] = uniform(rng, N, not full_scale)
    return x


# form -> (setup of q15_cases.SETUPS, batch, full-scale samples)
FORMS = {
    "none_b1": ("b1_rtl", 1, False),
    "none_b7_hann_u16": ("b1_hann_u16", 7, True),
    "none_b520_rom": ("b1_rom_rtl", 520, True),
    "none_b65": ("b1_rtl", 65, False),
    "default_b33": ("default", 33, False),
    "default_b65_rom_hann_u16": ("default_rom_hann_u16", 65, True),
    "default_b520": ("default", 520, False),
    "gui_b7": ("gui_upload", 7, False),
    "gui_b33_rom": ("gui_upload_rom", 33, True),
    "set12_b65_hann_u16": ("gui_upload_hann_u16", 65, True),
    "wide1_b1": ("wide1", 1, True),
    "wide2_b7_hann_u16": ("wide2_hann_u16", 7, False),
    "wide3_b33_rom": ("wide3_rom", 33, True),
    "wide4_b65": ("wide4", 65, False),
    "wide5_b7_rom_hann_u16": ("wide5_rom_hann_u16", 7, True),
    "wide6_b520_hann_u16": ("wide6_hann_u16", 520, False),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_mag_and_marker_equal_the_decoded_wire_frame(ch, torch_mod, oracle, form):
    """MAG == decode_mag_16iq_le(frame) and MARKER == (max, lo + argmax, int64 power sum) of it, bit for bit, on the
    oracle's frames: filter modes 0xB1, 0x00, 0xA1 (the GUI upload, which is fixture G4's `c_gui` and the 12-byte set of
    test_bit_exact_vs_integer_model), 0xA2 with the first 1..6 of wide_sections(); window modes 0 and 1; default and custom
    ROM; batches 1, 7, 33, 65 and 520; 12-bit and full-scale samples; every range of RANGES.  All-zero frames give
    (+0.0, lo, 0); the frames that are not all zero in are not all zero out."""
    setup, B, full = FORMS[form]
    rng = np.random.default_rng(1000 + list(FORMS).index(form))
    args = configure(ch, setup, rng)
    x = _samples(rng, B, full)
    ref = oracle.chain_q15(x, *args)
    assert all(ref[f].any() for f in range(B) if x[f].any()), form
    xd = to_device(torch_mod, x)
    _check_all(ch, torch_mod, xd, ref, tag=form)
    if B >= 7:                                                   # the all-zero frame, spelled out
        assert not ref[1].any()
        for lo, hi in RANGES:
            ch.set_marker_range(lo, hi)
            pm, pb, bp = _records(ch.process_q15(xd, out_kind="marker"))
            assert _bits(pm)[1] == 0 and pb[1] == lo and bp[1] == 0, (form, lo, hi)      # bits 0: a positive zero
    # the convenience views
    ch.set_marker_range(100, 9000)
    pm, pb, bp = ch.markers_q15(xd)
    pm2, pb2, bp2 = _records(ch.process_q15(xd, out_kind="marker"))
    assert pm.dtype == torch_mod.float32 and pb.dtype == torch_mod.int32 and bp.dtype == torch_mod.int64
    assert np.array_equal(_bits(pm.cpu().numpy()), _bits(pm2)) and np.array_equal(pb.cpu().numpy(), pb2)
    assert np.array_equal(bp.cpu().numpy(), bp2)


def test_extreme_frames(ch, torch_mod, oracle):
    """The frames of test_extreme_inputs (constant +/- full scale, alternating full scale, one full-scale impulse) in
    modes 0xB1 and 0x00 under the default ROM, then in mode 0xB1 under constant ROMs of either sign in both window
    modes (components down to -32767 on the oracle: no window setting passes -32768 itself), then through a saturating
    section in mode 0xA2 (b0 = 32767 in Q2.14, a gain of 2: the constant frames leave the cascade as -32768 / 32767), where
    bin 0 holds re = -32768 -- asserted on the oracle's frames, so the case cannot go missing: re^2 is 2^30 there,
    and a bin's integer power can reach 2^31, which fits uint32_t and not int32_t."""
    x = extreme_frames()
    xd = to_device(torch_mod, x)
    for cmd in (0xB1, 0x00):
        ch.set_filter_mode(cmd)
        _check_all(ch, torch_mod, xd, oracle.chain_q15(x, None, 0, cmd, None, None), tag=hex(cmd))
    sat = np.array([[32767, 0, 0, 16384, 0, 0]], np.int16)
    ch.load_sos_q14(sat)
    reached = 0
    for cmd in (0xB1, 0xA2):
        ch.set_filter_mode(cmd)
        for rom_v, wm in ((-32768, 0), (32767, 0), (32767, 1), (-32768, 1)):
            rom = np.full(N, rom_v, np.int16)
            ch.set_window_q15(rom)
            ch.set_window_mode_q15(wm)
            ref = oracle.chain_q15(x, rom, wm, cmd, None, sat)
            reached += int((ref == -32768).sum()) if cmd == 0xA2 else 0
            print(f"FIGURE extreme frames, mode 0x{cmd:02X} ROM {rom_v} window mode {wm}: components {ref.min()} .. {ref.max()}")
            _check_all(ch, torch_mod, xd, ref, tag=(cmd, rom_v, wm))
    assert reached >= 3, reached


def _full_scale_tones():
    """B = 512 single exact-bin cosines of amplitude 32767, bin in [1, 8192) and phase drawn per frame"""
    rng = np.random.default_rng(2)
    B = 512
    n = np.arange(N)
    bins = np.zeros(B, np.int64)
    x = np.zeros((B, N), np.int16)
    for f in range(B):
        bins[f] = rng.integers(1, 8192)
        ph = rng.uniform(0, 2 * np.pi)
        x[f] = np.rint(32767 * np.cos(2 * np.pi * bins[f] * n / N + ph)).astype(np.int16)
    return x, bins


def _tones_oracle(oracle):
    x, bins = _full_scale_tones()
    rom = np.full(N, 32767, np.int16)
    return x, bins, rom, oracle.chain_q15(x, rom, 0, 0xB1, None, None)


def test_rounding_cases_large_components(ch, torch_mod, oracle):
    """The evaluation order and the root are really tested: under the Hann ROM 12-bit samples give components of at most
    507, whose squares are exact and for which fma(r, r, q) has the same bits as fl(fl(r r) + q).  Here 512 full-scale
    exact-bin cosines pass an all-32767 ROM (window mode 0, filter 0xB1): on the oracle's frames at least 1000 bins have
    a component above 4096, and the models with one contracted square, sqrt(fl(fma(re, re, fl(im im)))) and the same
    with re and im exchanged, differ from decode_mag_16iq_le in at least 10 of those bins each -- asserted before the
    GPU result is looked at.  (Measured on the oracle: 1024 bins, values up to 16383; 15 / 19 bins change under the two
    contractions, 34 when the exact integer power is rounded once.)"""
    x, bins, rom, ref = _tones_oracle(oracle)
    mag, ip = _decode(ref)
    re, im = ref[..., 0], ref[..., 1]
    big = (np.abs(re.astype(np.int32)) > 4096) | (np.abs(im.astype(np.int32)) > 4096)
    assert big.sum() >= 1000, big.sum()
    r32, i32 = re.astype(np.float32), im.astype(np.float32)
    r64, i64 = re.astype(np.float64), im.astype(np.float64)
    # r r + fl(i i) is exact in float64 (below 2^53): rounding it to float32 is the single rounding of the FMA
    fma_re = np.sqrt((r64 * r64 + (i32 * i32).astype(np.float64)).astype(np.float32))
    fma_im = np.sqrt((i64 * i64 + (r32 * r32).astype(np.float64)).astype(np.float32))
    once = np.sqrt((r64 * r64 + i64 * i64).astype(np.float32))
    n_re, n_im, n_once = (int(((m != mag) & big).sum()) for m in (fma_re, fma_im, once))
    print(f"FIGURE rounding case: {int(big.sum())} bins above 4096 (max {int(np.abs(ref.astype(np.int32)).max())}); "
          f"contracted models differ in {n_re} (re) / {n_im} (im) bins, single rounding of the integer power in {n_once}")
    assert n_re >= 10 and n_im >= 10, (n_re, n_im)
    ch.set_window_q15(rom)
    ch.set_filter_mode(0xB1)
    _check_all(ch, torch_mod, to_device(torch_mod, x), ref, tag="tones")


def test_tie_rule_mirror_bins(ch, torch_mod, oracle):
    """Ties between k and N - k.  On this path the mirror bin is not always a bit-identical tie (per-stage truncation
    breaks the symmetry): in the batch of the rounding case at least 50 frames tie exactly on the full range (75 measured
    on the oracle) and report the tone's bin k < N/2; the other frames do NOT tie, and their record names whichever of
    k and N - k is larger -- both branches of the rule, against numpy's argmax on the decoded frame."""
    x, bins, rom, ref = _tones_oracle(oracle)
    mag, ip = _decode(ref)
    a = np.arange(len(bins))
    pk = mag.argmax(axis=1)
    assert (((pk == bins) | (pk == N - bins))).all()
    tie = mag[a, bins] == mag[a, N - bins]
    ntie = (mag == mag.max(axis=1)[:, None]).sum(axis=1)
    assert tie.sum() >= 50 and (ntie[tie] == 2).all() and (ntie[~tie] == 1).all(), (tie.sum(), ntie.max())
    assert (pk[tie] == bins[tie]).all()
    assert (pk[~tie] == N - bins[~tie]).any() and (pk[~tie] == bins[~tie]).any()
    print(f"FIGURE tie rule: {int(tie.sum())} of {len(bins)} frames tie exactly between k and N - k; "
          f"{int((pk == N - bins).sum())} frames peak at N - k")
    ch.set_window_q15(rom)
    ch.set_filter_mode(0xB1)
    ch.set_marker_range(0, N)
    pm, pb, bp = _records(ch.process_q15(to_device(torch_mod, x), out_kind="marker"))
    assert np.array_equal(pb[tie], bins[tie].astype(np.int32))
    assert np.array_equal(pb, pk.astype(np.int32))
    _check_marker(ch.process_q15(to_device(torch_mod, x), out_kind="marker"), mag, ip, 0, N, "tones")


def _sine_tones():
    """2048 exact-bin tones of amplitude 8300..16000 within 4e-4 rad of a pure +/- sine: the spectral line is
    (re ~ 0, im ~ +/- A/2) with A/2 above 4096, where float32 magnitudes are 4.9e-4 apart and a change of re^2 + im^2
    by 1 (re = 0 against re = +/- 1, same |im|) does not move the float"""
    rng = np.random.default_rng(3)
    B = 2048
    n = np.arange(N)
    bins = rng.integers(1, 8192, B)
    amp = rng.integers(8300, 16000, B)
    ph = np.where(rng.integers(0, 2, B) == 0, 0.5 * np.pi, -0.5 * np.pi) + rng.uniform(-4e-4, 4e-4, B)
    x = np.rint(amp[:, None] * np.cos(2 * np.pi * ((bins[:, None] * n[None, :]) % N) / N + ph[:, None])).astype(np.int16)
    return x, bins


def test_tie_rule_equal_floats_of_different_integer_powers(ch, torch_mod, oracle):
    """The comparison is on the float magnitudes: frames in which the LOWER bin k has the smaller integer power
    re^2 + im^2 but the same float32 magnitude as the higher bin N - k.  numpy's argmax on the decoded frame reports k;
    a search on the integer powers would report N - k.  Such frames are produced through the real chain (sine-phase
    tones whose line is (0, im) at k and (+/-1, -im) at N - k, |im| > 4096): the test asserts on the oracle's frames
    that at least 20 of the 2048 are of this kind (43 measured) before it looks at the GPU records."""
    x, bins = _sine_tones()
    rom = np.full(N, 32767, np.int16)
    ref = oracle.chain_q15(x, rom, 0, 0xB1, None, None)
    mag, ip = _decode(ref)
    a = np.arange(len(bins))
    kind = (mag[a, bins] == mag[a, N - bins]) & (ip[a, bins] < ip[a, N - bins])
    assert kind.sum() >= 20, kind.sum()
    assert (mag.argmax(axis=1)[kind] == bins[kind]).all() and (ip.argmax(axis=1)[kind] == N - bins[kind]).all()
    print(f"FIGURE tie rule: {int(kind.sum())} of {len(bins)} frames have equal floats of different integer powers at k and N - k")
    ch.set_window_q15(rom)
    ch.set_filter_mode(0xB1)
    xd = to_device(torch_mod, x)
    ch.set_marker_range(0, N)
    rec = ch.process_q15(xd, out_kind="marker")
    pm, pb, bp = _records(rec)
    assert np.array_equal(pb[kind], bins[kind].astype(np.int32))
    _check_marker(rec, mag, ip, 0, N, "sines")
    got = ch.process_q15(xd, out_kind="mag").cpu().numpy()
    assert np.array_equal(_bits(got), _bits(mag))


def test_config4_whole_batch_outputs(ch, torch_mod, oracle):
    """Config 4 as tests/test_gpu_q15.py::test_config4_whole_batch runs it (B = 4096, 12-bit samples of seed 2, the fixed
    ALPHA / BETA cascade of mode 0x00): the launch shape of the benchmark -- one cascade wave per SIMD, two FFT frames
    per CU.  MAG of every frame and MARKER on two ranges, against the decode of the oracle's frames."""
    torch = torch_mod
    gen = torch.Generator(device="cuda").manual_seed(2)
    B = 4096
    x = torch.randint(-2048, 2048, (B, N), generator=gen, device="cuda", dtype=torch.int32).to(torch.int16)
    ch.reserve(B)
    ch.set_filter_mode(0x00)
    magd = ch.process_q15(x, out_kind="mag").cpu().numpy()
    recs = []
    for lo, hi in ((0, N), (100, 9000)):
        ch.set_marker_range(lo, hi)
        recs.append(((lo, hi), ch.process_q15(x, out_kind="marker").cpu()))
    xh = x.cpu().numpy()
    for a in range(0, B, 512):                                         # the oracle in slices: bounded host memory
        ref = oracle.chain_q15(xh[a:a + 512], None, 0, 0x00, None, None)
        mag, ip = _decode(ref)
        bad = np.nonzero((_bits(magd[a:a + 512]) != _bits(mag)).any(axis=1))[0]
        assert bad.size == 0, f"MAG differs in frames {a + bad[:8]}"
        for (lo, hi), rec in recs:
            _check_marker(rec[a:a + 512], mag, ip, lo, hi, f"frames {a}..")


def test_records_are_reproducible_across_calls_overlap_and_graphs(ch, torch_mod):
    """Bit-identical records and magnitudes: repeated calls, overlap depths 2 and 3 (after flush) against the ordered
    mode, in mode 0xA2 (all of wide_sections(): the depth-2 ordering rule of the wide cascade, on frames that are not
    zero) and 0x00, and a torch.cuda.graph replay after reserve() against the eager call; a captured call keeps the range
    of capture time.  Launch timing reports one positive time per call for the new kinds."""
    torch = torch_mod
    rng = np.random.default_rng(31)
    xs = [to_device(torch, rng.integers(-2048, 2048, (600, N)).astype(np.int16)) for _ in range(4)]
    ch.reserve(600)
    for setup in ("wide6", "default"):
        configure(ch, setup)
        ch.set_marker_range(100, 9000)
        ref = [ch.process_q15(x, out_kind="marker").clone() for x in xs]
        refm = ch.process_q15(xs[0], out_kind="mag").clone()
        assert (refm != 0).any(dim=1).all().item(), setup                # every frame carries signal
        for _ in range(3):
            for x, r in zip(xs, ref):
                assert torch.equal(ch.process_q15(x, out_kind="marker"), r)
        for depth in (2, 3):
            ch.set_overlap(depth)
            outs = [ch.process_q15(x, out_kind="marker") for x in xs * 2]
            om = ch.process_q15(xs[0], out_kind="mag")
            ch.flush()
            torch.cuda.synchronize()
            for i, o in enumerate(outs):
                assert torch.equal(o, ref[i % 4]), (depth, i)
            assert torch.equal(om, refm), depth
            ch.set_overlap(1)
    ch.set_profiling(8)
    for x in xs:
        ch.process_q15(x, out_kind="marker")
        ch.process_q15(x, out_kind="mag")
    t = ch.profile_read(8)
    ch.set_profiling(0)
    assert len(t) == 8 and all(v > 0 for v in t), t
    out = torch.empty_like(ref[0])
    ch.process_q15(xs[0], out=out, out_kind="marker")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ch.process_q15(xs[0], out=out, out_kind="marker")
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref[0])
    # the captured call froze its range: a later change applies to eager calls only
    ch.set_marker_range(0, 50)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref[0])
    assert not torch.equal(ch.process_q15(xs[0], out_kind="marker"), ref[0])


def test_range_is_stream_ordered(ch, torch_mod, oracle):
    """Each call uses the range in force when it was issued, with no synchronisation between the calls, also at overlap
    depth 2; the float chain's marker calls use the same range of the handle."""
    torch = torch_mod
    rng = np.random.default_rng(9)
    x = rng.integers(-2048, 2048, (64, N)).astype(np.int16)
    ch.set_filter_mode(0x00)
    mag, ip = _decode(oracle.chain_q15(x, None, 0, 0x00, None, None))
    xd = to_device(torch, x)
    for depth in (1, 2):
        ch.set_overlap(depth)
        outs = []
        for lo, hi in RANGES:
            ch.set_marker_range(lo, hi)
            outs.append(ch.process_q15(xd, out_kind="marker"))
        ch.flush()
        torch.cuda.synchronize()
        for (lo, hi), rec in zip(RANGES, outs):
            _check_marker(rec, mag, ip, lo, hi, depth)
    ch.set_overlap(1)
    ch.set_marker_range(300, 700)
    assert ch.marker_range == (300, 700)
    pb = ch.process_f32(xd, out_kind="marker").cpu().numpy()[:, 1]
    assert ((pb >= 300) & (pb < 700)).all()


def test_refusals_leave_the_handle_usable(ch, torch_mod, oracle):
    """SA_EINVAL for a bad kind (wrapper and C entry point), a misaligned marker output and a NULL tensor, SA_ESHAPE for a
    wrong dtype or shape in the wrapper: nothing launched, and the next call is exact.  The 0xFF reset leaves the
    range alone.  process_q15(x) with no keyword returns the wire frames it returned before."""
    from fpga_real_time_fft_analyzer_amd import abi
    from fpga_real_time_fft_analyzer_amd.abi import SpecanError
    torch = torch_mod
    rng = np.random.default_rng(12)
    x = rng.integers(-2048, 2048, (4, N)).astype(np.int16)
    ref = oracle.chain_q15(x, None, 0, 0x00, None, None)
    mag, ip = _decode(ref)
    xd = to_device(torch, x)
    ch.set_filter_mode(0x00)
    ch.set_marker_range(300, 700)
    ch.set_profiling(64)

    def refused(code, fn):
        with pytest.raises(SpecanError) as e:
            fn()
        assert e.value.code == code, e.value
        _check_marker(ch.process_q15(xd, out_kind="marker"), mag, ip, 300, 700)

    refused(SA_EINVAL, lambda: ch.process_q15(xd, out_kind="mag_full"))
    bad = torch.empty(4 * 4 + 1, dtype=torch.int32, device="cuda")[1:].view(4, 4)
    refused(SA_EINVAL, lambda: ch.process_q15(xd, out=bad, out_kind="marker"))
    refused(SA_ESHAPE, lambda: ch.process_q15(xd, out=torch.empty((4, 4), dtype=torch.float32, device="cuda"), out_kind="marker"))
    refused(SA_ESHAPE, lambda: ch.process_q15(xd, out=torch.empty((4, N, 2), dtype=torch.int16, device="cuda"), out_kind="mag"))
    refused(SA_ESHAPE, lambda: ch.process_q15(xd, out=torch.empty((4, N), dtype=torch.float32, device="cuda"), out_kind="iq"))
    L = abi.lib()
    out = torch.empty((4, 4), dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    timed = len(ch.profile_read(64))
    assert timed == 5                               # the five good calls made after the refusals above, and no other
    for kind in (-1, 3, 99):
        assert L.sa_process_q15_out(ch._h, xd.data_ptr(), out.data_ptr(), 4, kind, stream) == SA_EINVAL
    assert L.sa_process_q15_out(ch._h, xd.data_ptr(), None, 4, 2, stream) == SA_EINVAL
    assert L.sa_process_q15_out(ch._h, None, out.data_ptr(), 4, 1, stream) == SA_EINVAL
    assert L.sa_process_q15_out(ch._h, xd.data_ptr(), out.data_ptr() + 4, 3, 2, stream) == SA_EINVAL
    assert len(ch.profile_read(64)) == timed        # no refused call was timed: no call state committed
    ch.set_profiling(0)
    _check_marker(ch.process_q15(xd, out_kind="marker"), mag, ip, 300, 700)
    # SA_Q15_OUT_IQ through the new entry point is sa_process_q15
    iq = torch.empty((4, N, 2), dtype=torch.int16, device="cuda")
    assert L.sa_process_q15_out(ch._h, xd.data_ptr(), iq.data_ptr(), 4, 0, stream) == 0
    assert np.array_equal(iq.cpu().numpy(), ref)
    assert np.array_equal(ch.process_q15(xd).cpu().numpy(), ref)
    assert ch.process_q15(xd).dtype == torch.int16 and ch.process_q15(xd).shape == (4, N, 2)
    ch.feed_command_bytes(b"\xff")
    assert ch.filter_mode == 0xB1 and ch.marker_range == (300, 700)
    _check_marker(ch.process_q15(xd, out_kind="marker"), *_decode(oracle.chain_q15(x)), 300, 700)
    e = torch.empty((0, N), dtype=torch.int16, device="cuda")
    assert ch.process_q15(e, out_kind="mag").shape == (0, N) and ch.process_q15(e, out_kind="marker").shape == (0, 4)


def test_frames_are_isolated(ch, torch_mod, oracle):
    """One frame of extreme samples between ordinary frames does not change the ordinary frames' records or magnitudes:
    they equal those of the same frames processed alone, in modes 0xB1, 0x00 and 0xA2 (all of wide_sections()), and in
    each of them every ordinary frame's magnitudes are not all zero."""
    torch = torch_mod
    rng = np.random.default_rng(44)
    x = rng.integers(-2048, 2048, (9, N)).astype(np.int16)
    ext = extreme_frames()
    ch.load_sos_q14(wide_sections())
    ch.set_marker_range(50, 16000)
    keep = [i for i in range(9) if i != 4]
    for cmd in (0xB1, 0x00, 0xA2):
        ch.set_filter_mode(cmd)
        alone_r = ch.process_q15(to_device(torch, x[keep]), out_kind="marker").cpu().numpy()
        alone_m = ch.process_q15(to_device(torch, x[keep]), out_kind="mag").cpu().numpy()
        assert alone_m.any(axis=1).all(), cmd
        for e in range(4):
            y = x.copy()
            y[4] = ext[e]
            yd = to_device(torch, y)
            assert np.array_equal(ch.process_q15(yd, out_kind="marker").cpu().numpy()[keep], alone_r), (cmd, e)
            assert np.array_equal(_bits(ch.process_q15(yd, out_kind="mag").cpu().numpy()[keep]), _bits(alone_m)), (cmd, e)
