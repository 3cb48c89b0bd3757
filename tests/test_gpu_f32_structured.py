"""GPU: the float path bin by bin and sample by sample, on structured inputs (impulses, exact-bin cosines, white noise,
steps) in every form the ABI reaches, against float64 references.

The parity tests of tests/test_gpu_f32.py bound the worst error of a tone frame's spectrum by 1e-5 of its peak, which
hides a defect in the bins away from the tone by three orders of magnitude (tests/structured_cases.py).  Here:
  - FFT: max_k |got - ref| / RMS_k |ref| per frame (bin_norm), bounded by max(1e-6, 4x scipy.fft.rfft in float32 on the
    same float32 windowed input);  ref = numpy.fft.rfft in float64 of the float32 input times the widened window.
  - cascade: max_n |y - ref| / max_n |ref| per frame, bounded by max(1e-5, 3x a sequential float32 sosfilt) on the
    float32 path and by 1e-6 with set_precision("f64");  ref = scipy.signal.sosfilt in float64.
  - scaling by powers of two: bit for bit (magnitudes: 1 ulp).
Every test prints its worst figure next to its bound (pytest -s); the first MI355X figures are in the docstrings.
"""
import numpy as np
import pytest
from scipy import signal

from conftest import N
from gpu_support import ch, table_window, to_device, torch_mod  # noqa: F401 (fixtures)
from structured_cases import CASCADE_VARIANTS, H, bin_norm, cascades, f32_fft_figure, fft_bound, plan_header

pytestmark = pytest.mark.gpu

IMPULSE_AT = [0, 1, 2, 3, 30, 31, 32, 33, 62, 63, 64, 65, 510, 511, 512, 513, 1022, 1023, 1024, 1025, 4095, 4096,
              8190, 8191, 8192, 8193, 16382, 16383]
COSINE_BINS = [0, 1, 2, 4095, 4096, 4097, 8191, 8192]
CASCADE_IMPULSE_AT = [0, 15, 16, 31, 32, 63, 64, 1023, 1024, 8191, 8192, 16383]
I16_AMP = 2048                        # impulse / cosine amplitude on the int16 entry: x = sample / 2048


def _fft_frames(i16, seed=0):
    """Impulses, exact-bin cosines and Hann-windowed white noise: (groups {name: slice}, x as float32 or int16)."""
    rng = np.random.default_rng(seed)
    n = np.arange(N)
    pos = IMPULSE_AT + sorted(rng.choice(N, 6, replace=False).tolist())
    bins = COSINE_BINS + sorted(rng.integers(3, 8190, 4).tolist())
    amp = I16_AMP if i16 else 1.0
    imp = np.zeros((len(pos), N))
    imp[np.arange(len(pos)), pos] = amp
    cos = np.stack([np.cos(2 * np.pi * ((k * n) % N) / N) for k in bins]) * (2047 if i16 else 1.0)
    hann = signal.windows.hann(N, sym=False)
    white = rng.standard_normal((8, N)) * hann * (400 if i16 else 1.0)
    x = np.concatenate([imp, cos, white])
    x = np.rint(x).astype(np.int16) if i16 else x.astype(np.float32)
    a, b = len(pos), len(pos) + len(bins)
    return {"impulse": slice(0, a), "cosine": slice(a, b), "white": slice(b, x.shape[0])}, x


# form -> (filter mode, identity sections, window, int16 entry, batch padded to, precision, expected (nsec, wingen))
FFT_FORMS = {
    "bypass_one_round": (0xB1, 0, "ones", False, None, "f32", (0, 0)),
    "bypass_two_round": (0xB1, 0, "ones", False, 513, "f32", (0, 0)),
    "bypass_int16": (0xB1, 0, "ones", True, None, "f32", (0, 0)),
    "identity1_nsec2": (0xA1, 1, "ones", False, None, "f32", (2, 1)),
    "identity2_nsec2": (0xA1, 2, "ones", False, None, "f32", (2, 1)),
    "identity3_nsec4": (0xA1, 3, "ones", False, None, "f32", (4, 1)),
    "identity4_nsec4": (0xA1, 4, "ones", False, None, "f32", (4, 1)),
    "identity5_nsec6": (0xA1, 5, "ones", False, None, "f32", (6, 1)),
    "identity6_nsec6": (0xA1, 6, "ones", False, None, "f32", (6, 1)),
    "identity6_table_window": (0xA1, 6, "table", False, None, "f32", (6, 0)),
    "identity2_int16": (0xA1, 2, "ones", True, None, "f32", (2, 1)),
    "identity2_f64": (0xA1, 2, "ones", False, None, "f64", (2, 1)),
}


def _setup(ch, mode, nident, window, precision):
    w = np.ones(N, np.float32) if window == "ones" else table_window()
    ch.set_window_f32(w)
    if nident:
        ch.load_sos(np.tile([1.0, 0, 0, 1.0, 0, 0], (nident, 1)))
    ch.set_filter_mode(mode)
    if precision != "f32":
        ch.set_precision(precision)
    return w


@pytest.mark.parametrize("form", list(FFT_FORMS))
def test_fft_bin_by_bin(ch, torch_mod, form):
    """Every output kind of the FFT, bin by bin: impulses on every digit boundary of the 32 x 16 x 16 complex FFT (both
    parities) -- ref w[n0] e^(-2 pi i k n0 / N) --, cosines at exact bins (leakage into every other bin; Im at DC and
    Nyquist, where the real-split step special-cases), Hann-windowed white noise.  Bound per input group:
    max(1e-6, 4x scipy's float32 rfft of the same float32 input).  spec_half, mag_half, mag_full (mirror bit for bit)
    and time (the windowed input, within one rounding).
    First MI355X run, worst of the twelve forms (bin norm; scipy float32 on the same input in brackets): impulses 4.1e-7
    (2.6e-7), exact-bin cosines 1.1e-5 (3.5e-6) and 1.3e-5 (5.2e-6) through the int16 entry, white noise 6.9e-7 (5.2e-7);
    Im at DC and Nyquist exactly 0 in every form; time exact (table window: 6.0e-8, the one rounding of x*w)."""
    mode, nident, window, i16, pad, precision, (want_nsec, want_wingen) = FFT_FORMS[form]
    w = _setup(ch, mode, nident, window, precision)
    if mode == 0xB1:
        assert ch.filter_mode == 0xB1 and want_nsec == 0           # bypass: no plan is launched
    else:
        nsec, unit, wingen, _ = plan_header(ch.iir_plan())
        assert (nsec, unit, wingen) == (want_nsec, 0, want_wingen)
    assert ch.precision == precision
    groups, x = _fft_frames(i16)
    B = x.shape[0]
    xin = np.concatenate([x, np.tile(x, (pad // B + 1, 1))[:pad - B]]) if pad else x
    x64 = x.astype(np.float64) / (I16_AMP if i16 else 1.0)
    xw64 = x64 * w.astype(np.float64)
    ref = np.fft.rfft(xw64, axis=1)
    xd = to_device(torch_mod, xin)
    kw = {"scale": 1.0 / I16_AMP} if i16 else {}
    out = {k: ch.process_f32(xd, out_kind=k, **kw).cpu().numpy()[:B] for k in ("spec_half", "mag_half", "mag_full", "time")}
    assert np.array_equal(out["mag_full"][:, H:], out["mag_full"][:, 1:H - 1][:, ::-1])
    assert np.array_equal(out["mag_full"][:, :H], out["mag_half"])
    worst = []
    for g, sl in groups.items():
        r = ref[sl]
        f32 = f32_fft_figure(xw64[sl].astype(np.float32), r)
        bound = fft_bound(xw64[sl].astype(np.float32), r)
        e_spec = bin_norm(out["spec_half"][sl], r)
        e_mag = bin_norm(out["mag_half"][sl], np.abs(r))
        rms = np.sqrt(np.mean(np.abs(r) ** 2, axis=1))
        e_dc_ny = float((np.abs(out["spec_half"][sl][:, [0, H - 1]].imag).max(axis=1) / rms).max())
        worst.append((g, e_spec, e_mag, e_dc_ny, f32, bound))
        print(f"FIGURE fft {form} {g}: spec {e_spec:.2e} mag {e_mag:.2e} Im(DC,Nyq) {e_dc_ny:.2e} "
              f"| scipy float32 {f32:.2e} bound {bound:.2e}")
    # time output: the windowed input (one float32 rounding of x*w; f64 precision: y = x*w rounded once)
    t_err = float((np.abs(out["time"] - xw64) / np.maximum(np.abs(xw64), 1e-30)).max(where=xw64 != 0, initial=0.0))
    assert not np.any(out["time"][xw64 == 0]), "time output nonzero where the input is zero"
    print(f"FIGURE fft {form} time: max relative {t_err:.2e}")
    for g, e_spec, e_mag, e_dc_ny, f32, bound in worst:
        assert e_spec <= bound and e_mag <= bound and e_dc_ny <= bound, (form, g, e_spec, e_mag, e_dc_ny, f32, bound)
    assert t_err <= 2.0 ** -23, (form, t_err)


def _cascade_frames(rng):
    pos = CASCADE_IMPULSE_AT + sorted(rng.choice(np.arange(1, N), 4, replace=False).tolist())
    x = np.zeros((len(pos) + 1, N), np.float32)
    x[np.arange(len(pos)), pos] = 1.0
    x[-1] = 1.0                                              # step: accumulates over all 16 rows
    return pos, x


def _run_cascade(ch, torch_mod, name, sos, precision):
    w = np.ones(N, np.float32)
    ch.set_window_f32(w)
    if name == "smoother_f32":
        ch.load_sos_f32(sos)
    else:
        ch.load_sos(sos)
    ch.set_filter_mode(0xA1)
    if precision == "f64":
        ch.set_precision("f64")
    nsec, unit, wingen, _ = plan_header(ch.iir_plan())
    assert (nsec, unit, wingen) == (CASCADE_VARIANTS[name][0], CASCADE_VARIANTS[name][1], 1)
    pos, x = _cascade_frames(np.random.default_rng(sum(map(ord, name))))
    xd = to_device(torch_mod, x)
    y = ch.process_f32(xd, out_kind="time").cpu().numpy().astype(np.float64)
    spec = ch.process_f32(xd, out_kind="spec_half").cpu().numpy()
    ref = signal.sosfilt(sos, x.astype(np.float64), axis=1)
    from oracle import oracle as orc
    seq = np.stack([orc.sosfilt_f32_c(sos, r) for r in x]).astype(np.float64)
    return pos, y, spec, ref, seq


def _peak_rel(got, ref):
    return np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("name", list(CASCADE_VARIANTS))
def test_cascade_sample_by_sample(ch, torch_mod, oracle, name, precision):
    """Impulse responses starting at the chunk (32), thread (64), row (1024) and half-frame (8192) boundaries and at
    random positions, plus a step, through every cascade of the CPU coverage table (test_plan_conditioning pins the
    kernel variant each reaches), flat window.  time output per frame within max(1e-5, 3x a sequential float32 sosfilt)
    of the float64 sosfilt (f64 precision: 1e-6); the spectrum in the per-bin norm within the same factor of the
    sequential float32 spectrum (f64: the float32-FFT bound).  Time invariance without a reference: the response to
    an impulse at n0, shifted back by n0, matches the response at 0 within the same bound.
    First MI355X run: float32 time error at most 1.3x the sequential float32 figure (fast_real, 6.5e-8 against 4.9e-8;
    near_double 5.4e-6 against 6.9e-6; long_memory 4.9e-5 against 5.9e-3), spectrum within 0.6x of its bound; f64 precision
    time error at most 5.9e-8, spectrum at most 7.1e-6 against a float32-FFT bound of 2.8e-5, shift error 0 or ~1e-8."""
    sos = cascades()[name]
    pos, y, spec, ref, seq = _run_cascade(ch, torch_mod, name, sos, precision)
    e_t = _peak_rel(y, ref)
    R = np.fft.rfft(ref, axis=1)
    if precision == "f32":
        s_t = _peak_rel(seq, ref)
        b_t = np.maximum(1e-5, 3 * s_t)
        b_s = np.array([max(1e-5, 3 * bin_norm(np.fft.rfft(seq[i]), R[i])) for i in range(len(R))])
    else:
        b_t = np.full(len(ref), 1e-6)
        b_s = np.array([max(1e-6, fft_bound(ref[i].astype(np.float32), R[i])) for i in range(len(R))])
    e_s = np.array([bin_norm(spec[i], R[i]) for i in range(len(R))])
    i0 = pos.index(0)
    shift = max(float(np.abs(y[i][n0:] - y[i0][:N - n0]).max() / np.abs(y[i0]).max()) for i, n0 in enumerate(pos))
    print(f"FIGURE cascade {name} {precision}: time {e_t.max():.2e} (bound {b_t[np.argmax(e_t)]:.2e}, "
          f"sequential f32 {_peak_rel(seq, ref).max():.2e}) spectrum {e_s.max():.2e} (bound {b_s[np.argmax(e_s)]:.2e}) "
          f"shift {shift:.2e}")
    assert (e_t <= b_t).all(), [(pos[i] if i < len(pos) else "step", e_t[i], b_t[i]) for i in np.flatnonzero(e_t > b_t)]
    assert (e_s <= b_s).all(), [(pos[i] if i < len(pos) else "step", e_s[i], b_s[i]) for i in np.flatnonzero(e_s > b_s)]
    assert shift <= 2 * b_t[i0], shift


SCALE_FORMS = {"bypass": (0xB1, None, "f32"), "butter12": (0xA1, "butter12", "f32"), "rtl_default": (0xA1, "rtl_default", "f32"),
               "butter12_f64": (0xA1, "butter12", "f64")}


@pytest.mark.parametrize("form", list(SCALE_FORMS))
def test_power_of_two_scaling_is_exact(ch, torch_mod, form):
    """Every operation on the float path is linear in the input, so scaling the input by 2^k scales spec_half and time
    by exactly 2^k, bit for bit (include/specan.h states the range); magnitudes within 1 ulp (sqrt rounding).  The int16
    entry with scale 2^k / 2048 against scale 1 / 2048 the same.  First MI355X run: exact for every k and form."""
    mode, casc, precision = SCALE_FORMS[form]
    if casc:
        ch.load_sos(cascades()[casc])
    ch.set_filter_mode(mode)
    if precision == "f64":
        ch.set_precision("f64")
    rng = np.random.default_rng(4)
    n = np.arange(N)
    x = (0.5 * np.sin(2 * np.pi * 0.0123 * n) + 0.3 * rng.standard_normal((4, N))).astype(np.float32)
    xi = rng.integers(-2048, 2048, size=(3, N)).astype(np.int16)
    kinds = ("spec_half", "time", "mag_full")
    base = {k: ch.process_f32(to_device(torch_mod, x), out_kind=k).cpu().numpy() for k in kinds}
    base_i = {k: ch.process_f32(to_device(torch_mod, xi), out_kind=k, scale=1.0 / 2048).cpu().numpy() for k in kinds}
    for k2 in (-30, -8, 8, 30):
        s = np.float32(2.0 ** k2)
        got = {k: ch.process_f32(to_device(torch_mod, x * s), out_kind=k).cpu().numpy() for k in kinds}
        got_i = {k: ch.process_f32(to_device(torch_mod, xi), out_kind=k, scale=2.0 ** k2 / 2048).cpu().numpy() for k in kinds}
        for g, b in ((got, base), (got_i, base_i)):
            assert np.array_equal(g["spec_half"], b["spec_half"] * s), (form, k2)
            assert np.array_equal(g["time"], b["time"] * s), (form, k2)
            want = b["mag_full"] * s
            assert (np.abs(g["mag_full"] - want) <= np.spacing(want)).all(), (form, k2)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_real_pole_pair_family(ch, precision):
    """200 cascades of the real-pole-pair fuzz family (tests/fuzz_parity.py, random_real_pair_sos: near-double pairs with
    gaps 0 .. 1e-1, first-order sections, separated real pairs, mixed with Butterworth sections) x tones + noise, in
    the norm of test_random_designs: float32 within max(1e-5, 4x sequential float32), f64 precision within 1e-5 flat.
    First MI355X run: float32 worst 4.1e-6 (sequential float32 1.9e-6), f64 worst 2.2e-7."""
    import fuzz_parity
    if precision == "f64":
        ch.set_precision("f64")
    res = fuzz_parity.sweep(ch, 3, 200, family="real")
    assert len(res) == 200
    bound = (lambda seq: max(1e-5, 4 * seq)) if precision == "f32" else (lambda seq: 1e-5)
    worst = max(res, key=lambda r: r[0] / bound(r[2]))
    print(f"FIGURE real family {precision}: worst {worst[0]:.2e} (sequential f32 {worst[2]:.2e}) {worst[3]}")
    bad = [(err, seq, label) for err, _, seq, label in res if not err <= bound(seq)]
    assert not bad, sorted(bad, reverse=True)[:5]
