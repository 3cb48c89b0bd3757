"""GPU: the fold of float magnitudes over groups of A = 2^a frames and buckets of W = 2^k bins (include/specan_fold.h:
sa_fold_mag_f32 of libspecan_fold.so), through SpectrumChain.fold_mag_f32, SpectrumChain.spectra_f32 and the C entry point.

Every comparison but one is exact, on float bits, against the numpy mirror frames.fold_of_mags, whose order of summation
tests/test_f32_fold_cpu.py pins with probes worked out by hand; those probes are part of the data here, and their bits are
asserted again on the device's records.  A NaN power is compared by isnan, as the header specifies no payload.  The one
tolerance is the project's parity bound, 1e-5 in the max-norm per row, of the Welch estimate against float64."""
import numpy as np
import pytest

from conftest import N, load_golden, rel_maxnorm
from gpu_support import ch, synth, to_device, torch_mod  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

SA_OK, SA_EINVAL, SA_ESHAPE = 0, -1, -2
# squares 1, 2^-24, 0, 0 and four times 2^-54: the balanced pair tree gives 1 + 2^-24 + 2^-52 -> 0x3F800001, a sequential sum
# 1 + 2^-24, the tie that goes to the even 0x3F800000 (tests/test_f32_fold_cpu.py derives both)
PROBE = np.array([1.0, 2.0 ** -12, 0.0, 0.0, 2.0 ** -27, 2.0 ** -27, 2.0 ** -27, 2.0 ** -27], np.float32)
SPECIAL = 640                                                    # the bins [0, 640) of every frame hold the cases below
# A >= 2, the first two frames of a group: per bin over the frames c = (1 + 2^-24, 0, 2^-53, 2^-53); the pair tree (c0 + c1) +
# (c2 + c3) = 1 + 2^-24 + 2^-52 -> 0x3F800001; a sequential ((c0 + c1) + c2) + c3 meets two ties that go to the even
# 1 + 2^-24 -> 0x3F800000, and so does summing a frame's bins before the frames (tests/test_f32_fold_cpu.py derives it)
QUAD = np.array([[1.0, 0.0, 2.0 ** -27, 2.0 ** -27], [2.0 ** -12, 0.0, 2.0 ** -27, 2.0 ** -27]], np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _mags(A, seed):
    """[2A, N] magnitudes: exp of a uniform over +-60 (wide in exponent; squares past float32 from e^44 on), and in the first
    640 bins, each case alone in a zeroed block of 64 bins so that it is alone in its record at every W:
      block 0  the bin probe in bins 0..7 of each group's first frame;
      block 1  the frame probe down bin 64 over the first min(A, 8) frames of each group;
      block 2  2^-70 (power 2^-140, a float32 denormal);   block 3  2^-140 (a denormal input; power +0);
      block 4  3e38 (power +inf, finite peak);             block 5  -0.0 in every frame;
      block 6  a NaN, block 7 a +inf, both in group 0 only;
      block 8  (A >= 2) the quad probe in bins 512..515 of each group's first two frames: the four bins of one thread, lane 0
               of its bucket at every W >= 8;
      block 9  (A >= 2) the same in bins 580..583: one thread again, and at W >= 8 NOT the bucket's lowest lane, so its sum
               reaches the record through the lanes."""
    rng = np.random.default_rng(seed)
    m = np.exp(rng.uniform(-60.0, 60.0, size=(2 * A, N))).astype(np.float32)
    m[:, :SPECIAL] = 0.0
    for g in (0, A):
        m[g, 0:8] = PROBE
        n = min(A, 8)
        m[g:g + n, 64] = PROBE[:n]
        m[g + A - 1, 128] = 2.0 ** -70
        m[g, 192] = 2.0 ** -140
        m[g + A // 2, 256] = 3e38
        m[g:g + A, 320:384] = -0.0
        if A >= 2:
            m[g:g + 2, 512:516] = QUAD
            m[g:g + 2, 580:584] = QUAD
    m[A - 1, 384 + 5] = np.nan
    m[0, 448 + 63] = np.inf
    return m


def _same(rec, peak, power, tag):
    """a [G, P, 2] float32 record array against the mirror: bits, and isnan where the mirror's power is a NaN"""
    assert rec.shape == peak.shape + (2,) and rec.dtype == np.float32, (tag, rec.shape, rec.dtype)
    bad = np.nonzero(_bits(rec[..., 0]) != _bits(peak))
    assert bad[0].size == 0, (tag, "peak", bad[0][:5], bad[1][:5], _bits(rec[..., 0])[bad][:5], _bits(peak)[bad][:5])
    nan = np.isnan(power)
    assert np.array_equal(np.isnan(rec[..., 1]), nan), (tag, "power NaN")
    bad = np.nonzero((_bits(rec[..., 1]) != _bits(power)) & ~nan)
    assert bad[0].size == 0, (tag, "power", bad[0][:5], bad[1][:5], _bits(rec[..., 1])[bad][:5], _bits(power)[bad][:5])


@pytest.mark.parametrize("a", range(8))
def test_every_pair_equals_the_mirror(ch, torch_mod, a):
    """All 55 (a, k): B = 2A, two groups; both fields of every record by bits against frames.fold_of_mags, and the hand-made
    cases by their own expected bits."""
    from fpga_real_time_fft_analyzer_amd import frames
    A = 1 << a
    m = _mags(A, 1500 + a)
    md = to_device(torch_mod, m)
    for k in range(7):
        if (a, k) == (0, 0):
            continue
        W, tag = 1 << k, (a, k)
        rec = ch.fold_mag_f32(md, A, W).cpu().numpy()
        peak, power, _ = frames.fold_of_mags(m, A, W)
        _same(rec, peak, power, tag)
        pk, pw = _bits(rec[..., 0]), _bits(rec[..., 1])
        for g in (0, 1):
            if k == 3:                                           # the bin probe is one record: the tree's bits
                assert pw[g, 0] == 0x3F800001 and pk[g, 0] == 0x3F800000, tag
            if k == 0 and a >= 3:                                # the frame probe is one record: the sequential sum's bits
                assert pw[g, 64] == 0x3F800000 and pk[g, 64] == 0x3F800000, tag
            assert (pk[g, 128 >> k], pw[g, 128 >> k]) == ((127 - 70) << 23, 0x200), tag
            assert (pk[g, 192 >> k], pw[g, 192 >> k]) == (0x200, 0), tag
            assert pw[g, 256 >> k] == 0x7F800000 and pk[g, 256 >> k] == _bits(np.float32(3e38))[0], tag
            assert not pk[g, 320 >> k:384 >> k].any() and not pw[g, 320 >> k:384 >> k].any(), tag
            if k >= 2 and a >= 1:                                # the quad probe is one record: the in-thread tree's bits,
                for j in (512 >> k, 580 >> k):                   # in the bucket's lowest lane and in another one
                    assert (pk[g, j], pw[g, j]) == (0x3F800000, 0x3F800001), (tag, j)
        j = (384 + 5) >> k
        assert np.isnan(rec[0, j]).all() and np.isfinite(rec[1, j]).all() and np.isfinite(rec[0, j - 1]).all(), tag
        j = (448 + 63) >> k
        assert (pk[0, j], pw[0, j]) == (0x7F800000, 0x7F800000) and np.isfinite(rec[1, j]).all(), tag


@pytest.mark.parametrize("a,k", [(0, 1), (0, 6), (2, 0), (1, 2), (3, 3), (7, 6)])
def test_poisoned_out_and_a_guard_behind_it(ch, torch_mod, a, k):
    """`out` and a guard region behind it hold 0xFF bytes: every record is written (no peak has its sign bit, and no power of
    this data is a NaN), and nothing outside (B / A) (16384 / W) 8 bytes is touched."""
    from fpga_real_time_fft_analyzer_amd import frames
    torch = torch_mod
    A, W, B = 1 << a, 1 << k, 3 << a
    m = synth(B, 1600 + 8 * a + k)
    m = np.abs(m)
    md = to_device(torch, m)
    n_out = (B // A) * (N // W) * 8
    buf = torch.full((n_out + 4096,), 0xFF, dtype=torch.uint8, device="cuda")
    out = buf[:n_out].view(torch.float32).view(B // A, N // W, 2)
    assert ch.fold_mag_f32(md, A, W, out=out) is out
    torch.cuda.synchronize()
    assert (buf[n_out:] == 0xFF).all().item()
    rec = out.cpu().numpy()
    assert (_bits(rec) != 0xFFFFFFFF).all()
    _same(rec, *frames.fold_of_mags(m, A, W)[:2], (a, k))


def _inputs(torch, rng, B):
    """the three input forms of one batch of 12-bit samples: float32 (sample / 2048), int16, packed uint8"""
    from fpga_real_time_fft_analyzer_amd.ingest import pack12
    n = np.arange(N)
    xi = np.clip(np.rint(1500.0 * np.sin(2 * np.pi * rng.uniform(0.01, 0.45, (B, 1)) * n) + 100.0 * rng.standard_normal((B, N))),
                 -2048, 2047).astype(np.int16)
    return {"float32": to_device(torch, (xi / 2048.0).astype(np.float32)), "int16": to_device(torch, xi),
            "uint8": to_device(torch, pack12(xi))}


PAIRS = ((4, 1), (1, 16), (4, 16), (8, 64))


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("mode", [0xB1, 0xA1])
def test_spectra_f32_is_the_fold_of_process_f32(ch, torch_mod, mode, precision):
    """x float32, int16 and packed uint8; mode 0xB1, and 0xA1 with the six sections of G2; both precisions; B = 8: the call
    equals fold_of_mags(process_f32(x, 'mag_full')) bit for bit -- stream-ordered, with a caller's `work`, and at overlap
    depth 2 with the input and the workspace dropped and their memory scribbled over right behind the call."""
    from fpga_real_time_fft_analyzer_amd import frames
    torch = torch_mod
    B = 8
    if mode == 0xA1:
        ch.load_sos(load_golden("g2_config1.npz")["sos"])
    ch.set_filter_mode(mode)
    ch.set_precision(precision)
    for form, x in _inputs(torch, np.random.default_rng(1700 + mode), B).items():
        mag = ch.process_f32(x, out_kind="mag_full").cpu().numpy()
        assert mag.any() and np.isfinite(mag).all()
        want = {p: frames.fold_of_mags(mag, *p)[:2] for p in PAIRS}
        for p in PAIRS:
            _same(ch.spectra_f32(x, *p).cpu().numpy(), *want[p], (form, p, "ordered"))
            work = torch.full((B + 1, N), 3.0, dtype=torch.float32, device="cuda")
            _same(ch.spectra_f32(x, *p, work=work).cpu().numpy(), *want[p], (form, p, "work"))
            assert np.array_equal(work[:B].cpu().numpy(), mag) and (work[B] == 3.0).all().item()
        ch.set_overlap(2)
        for p in PAIRS:
            x2, work = x.clone(), torch.empty((B, N), dtype=torch.float32, device="cuda")
            rec = ch.spectra_f32(x2, *p, work=work)
            del x2, work                                         # free again when the call returns: the allocator hands
            scribble = [torch.full((B, N), 7e7, dtype=torch.float32, device="cuda"),       # their blocks out again
                        torch.full(x.shape, 85, dtype=x.dtype, device="cuda")]
            torch.cuda.synchronize()
            _same(rec.cpu().numpy(), *want[p], (form, p, "overlap 2"))
            rec = ch.spectra_f32(x, *p)                          # and with the cached workspace
            torch.cuda.synchronize()
            _same(rec.cpu().numpy(), *want[p], (form, p, "overlap 2, cached"))
            del scribble
        ch.set_overlap(1)


def test_welch_estimate_of_g3(ch, torch_mod, oracle):
    """G3 frames, bypass: power / group of spectra_f32 against the float64 mean of |rfft(x hann)|^2 mirrored to 16384 bins, in
    the project's parity norm (max-norm relative per row) and bound (1e-5)."""
    x = load_golden("g3_fp32_frames.npz")["x"]
    _, _, mag = oracle.chain_fp(x, None)
    for group in (4, 8):
        ref = (mag ** 2).reshape(8 // group, group, N).mean(axis=1)
        rec = ch.spectra_f32(to_device(torch_mod, x), group).cpu().numpy()
        err = rel_maxnorm(rec[..., 1].astype(np.float64) / group, ref)
        print(f"FIGURE welch group {group}: max-norm relative error {err:.3e}")
        assert err <= 1e-5, (group, err)
        top = rel_maxnorm(rec[..., 0], mag.reshape(8 // group, group, N).max(axis=1))
        assert top <= 1e-5, (group, top)


def test_refusals_through_the_library(ch, torch_mod):
    """Misaligned slices, an `out` that meets `mag`, B no multiple of A: the C call gives the code sa_fold_check gives for the
    same integers, with its text, and writes nothing; through the wrapper the same codes, and a good call afterwards."""
    from fpga_real_time_fft_analyzer_amd import abi, frames
    from fpga_real_time_fft_analyzer_amd.abi import SpecanError
    torch = torch_mod
    L = abi.fold_lib()
    stream = torch.cuda.current_stream().cuda_stream
    B, a, k = 8, 2, 4
    n_out = (B >> a) * (N >> k) * 2                                              # floats
    m = np.abs(synth(B, 1800))
    flat = torch.zeros((B * N + 4 + n_out,), dtype=torch.float32, device="cuda")
    flat[:B * N] = to_device(torch, m).view(-1)
    mag = flat[:B * N].view(B, N)
    canary = 7.0
    out = torch.full((B >> a, N >> k, 2), canary, dtype=torch.float32, device="cuda")
    off = torch.full((n_out + 4,), canary, dtype=torch.float32, device="cuda")
    before = flat.clone()
    cases = [("mag 4 bytes off", flat[1:1 + B * N].data_ptr(), out.data_ptr(), B, SA_EINVAL, "`mag` must be 16-byte aligned"),
             ("out 8 bytes off", mag.data_ptr(), off[2:].data_ptr(), B, SA_EINVAL, "`out` must be 16-byte aligned"),
             ("out inside mag", mag.data_ptr(), flat[B * N - 4:].data_ptr(), B, SA_EINVAL, "overlap"),
             ("mag inside out", flat[n_out - 4:].data_ptr(), flat.data_ptr(), B, SA_EINVAL, "overlap"),
             ("in place", mag.data_ptr(), mag.data_ptr(), B, SA_EINVAL, "overlap"),
             ("B % A", mag.data_ptr(), out.data_ptr(), B - 2, SA_ESHAPE, "multiple"),
             ("B % A before NULL", 0, 0, B + 1, SA_ESHAPE, "multiple"),
             ("NULL", mag.data_ptr(), 0, B, SA_EINVAL, "NULL"),
             ("both 0", mag.data_ptr(), out.data_ptr(), B, None, "folds nothing"),
             ("negative", mag.data_ptr(), out.data_ptr(), -4, SA_ESHAPE, "negative")]
    for tag, pin, pout, batch, code, words in cases:
        aa, kk = (0, 0) if code is None else (a, k)
        want = L.sa_fold_check(aa, kk, pin, pout, batch)
        assert want == (SA_EINVAL if code is None else code), tag
        assert L.sa_fold_mag_f32(pin, pout, batch, aa, kk, stream) == want, tag
        assert words in L.sa_fold_last_error().decode(), (tag, L.sa_fold_last_error())
    torch.cuda.synchronize()
    assert (out == canary).all().item() and (off == canary).all().item() and torch.equal(flat, before)
    assert L.sa_fold_mag_f32(0, 0, 0, a, k, stream) == SA_OK and L.sa_fold_last_error() == b""
    # `out` right behind `mag` touches it: fine
    touch = flat[B * N:B * N + n_out].view(B >> a, N >> k, 2)
    assert L.sa_fold_mag_f32(mag.data_ptr(), touch.data_ptr(), B, a, k, stream) == SA_OK
    peak, power, _ = frames.fold_of_mags(m, 1 << a, 1 << k)
    _same(touch.cpu().numpy(), peak, power, "touching")

    def refused(code, *args, **kw):
        with pytest.raises(SpecanError) as e:
            ch.fold_mag_f32(*args, **kw)
        assert e.value.code == code, (args, kw, str(e.value))
        return str(e.value)

    assert "16-byte aligned" in refused(SA_EINVAL, mag, 4, 16, out=off[2:2 + n_out].view(B >> a, N >> k, 2))
    assert "bytes read" in refused(SA_EINVAL, mag, 4, 16, out=flat[B * N - 4:B * N - 4 + n_out].view(B >> a, N >> k, 2))
    refused(SA_ESHAPE, mag[:6], 4, 16)
    refused(SA_ESHAPE, mag, 4, 16, out=torch.empty((B >> a, N >> k), dtype=torch.float32, device="cuda"))
    refused(SA_ESHAPE, mag[:, :N // 2], 4, 16)
    refused(SA_EINVAL, mag.double(), 4, 16)
    refused(SA_EINVAL, mag, 1, 1)
    with pytest.raises(SpecanError) as e:
        ch.spectra_f32(mag[:6], 4)
    assert e.value.code == SA_ESHAPE
    with pytest.raises(SpecanError) as e:
        ch.spectra_f32(mag, 4, work=torch.empty((B - 1, N), dtype=torch.float32, device="cuda"))
    assert e.value.code == SA_ESHAPE
    torch.cuda.synchronize()
    assert (out == canary).all().item() and (off == canary).all().item()
    _same(ch.fold_mag_f32(mag, 4, 16, out=out).cpu().numpy(), peak, power, "the good call")
    assert ch.fold_mag_f32(torch.empty((0, N), dtype=torch.float32, device="cuda"), 128, 64).shape == (0, N // 64, 2)


def test_capture_and_replay(ch, torch_mod):
    """Depth 1: after one warm-up call of the same batch (it allocates the cached workspace) spectra_f32 is captured -- both of
    its launches go to the capturing stream one behind the other, a serial chain -- and replayed on new input: the eager
    result of that input, bit for bit.  The fold alone captures without a warm-up."""
    torch = torch_mod
    B, p = 8, (4, 16)
    assert ch.overlap == 1                                       # both launches go to the capturing stream: no fork, no join
    xs = [to_device(torch, synth(B, 1900 + i)) for i in range(2)]
    x = xs[0].clone()
    eager = [ch.spectra_f32(xi, *p).clone() for xi in xs]
    assert not torch.equal(eager[0], eager[1])
    out = torch.zeros_like(eager[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ch.spectra_f32(x, *p, out=out)
    for i in (1, 0):
        x.copy_(xs[i])
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), eager[i].view(torch.int32)), i
    mag = ch.process_f32(xs[1], out_kind="mag_full")
    out2 = torch.zeros_like(out)
    graph2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph2):
        ch.fold_mag_f32(mag, *p, out=out2)
    graph2.replay()
    torch.cuda.synchronize()
    assert torch.equal(out2.view(torch.int32), eager[1].view(torch.int32))
    assert "libspecan_fold.so" in open("/proc/self/maps").read()
