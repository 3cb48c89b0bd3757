"""GPU: the window the float chain applies, held to the loaded table per sample and per bin, in every device layout and
kernel form that reads or generates it (tests/window_cases.py: the windows, A(w), the frames, the form table, the gates).

  T1  table paths (bypass, identity cascades on a refused window, f64 precision): 'time' = x w within 2^-23 relative,
      exactly 0 where x w is 0, the right sign at the negative entries.
  T2  identity cascades on an accepted window: |time - x w| <= A(w) peak |x| + 2^-24 |x w| per sample.  ('time' reads the
      plan's table copy of the window; the generator is evaluated by the spectrum kernels: T3.)
  T3  spec_half and mag_half of the noise and the impulse frame against numpy's float64 rfft of x w, w the loaded table:
      structured_cases.bin_norm within fft_bound, plus A(w) peak sqrt(N) rms(x) / RMS_k |ref| under a generated window;
      mag_full mirrors bit for bit.
  T4  real cascades (mode 0x00, unit-numerator forms, f64 butter12): 'time' and spec_half against float64 sosfilt + rfft
      of x w within the bounds of test_gpu_f32_structured.test_cascade_sample_by_sample.
  T5  every order of the control calls reaches the state of a fresh handle, bit for bit.
  T6  a window scaled by 2^k keeps its verdict and scales the outputs by exactly 2^k.
Every test prints its worst figure next to its bound (pytest -s); the first MI355X figures are in the docstrings."""
import numpy as np
import pytest
from scipy import signal

import structured_cases as sc
import window_cases as wc
from gpu_support import ch, to_device, torch_mod  # noqa: F401 (fixtures)
from window_cases import FORMS, H

pytestmark = pytest.mark.gpu


def _configure(ch, fm, window, scale=1.0):
    """The form's control calls, window first; asserts the plan the form expects.  Returns the table, widened."""
    w = wc.loaded(window)
    ch.set_window_f32(w if w is None or scale == 1.0 else w * np.float32(scale))
    sos = wc.cascade_sos(fm.cascade)
    if sos is not None:
        ch.load_sos(sos)
    ch.set_filter_mode(fm.mode)
    if fm.precision == "f64":
        ch.set_precision("f64")
    assert ch.filter_mode == fm.mode and ch.precision == fm.precision
    if fm.nsec:
        nsec, unit, wingen, _ = sc.plan_header(ch.iir_plan())
        assert (nsec, unit, wingen) == (fm.nsec, fm.unit, int(wc.VERDICTS[window])), (window, nsec, unit, wingen)
    return wc.table(window).astype(np.float64) * scale


def _input(torch_mod, fm):
    """(device tensor in the form's input type, padded as the form asks; x widened [4, N]; keyword arguments of the call)."""
    integer = fm.in_form != "float32"
    x, x64 = wc.frames(integer)
    if fm.in_form == "uint8":
        from fpga_real_time_fft_analyzer_amd.ingest import pack12
        x = pack12(x)
    if fm.pad:
        x = np.concatenate([x, np.tile(x, (fm.pad // 4 + 1, 1))[:fm.pad - 4]])
    return to_device(torch_mod, x), x64, ({"scale": wc.INT_SCALE} if integer else {})


def _outputs(ch, xd, kw, kinds=wc.KINDS):
    return {k: ch.process_f32(xd, out_kind=k, **kw).cpu().numpy()[:4] for k in kinds}


def _mirror_ok(out):
    return (np.array_equal(out["mag_full"][:, H:], out["mag_full"][:, 1:H - 1][:, ::-1])
            and np.array_equal(out["mag_full"][:, :H], out["mag_half"]))


@pytest.mark.parametrize("form", [f for f, fm in FORMS.items() if fm.gate in ("T1", "T1/T2")])
def test_applied_window_per_sample_and_per_bin(ch, torch_mod, form):
    """T1 / T2 on all four frames and T3 on the noise and the impulse frame, for every window of the form: the bypass
    forms (float32 in one round and, at B = 513, in two; int16; packed 12-bit: win_b and win_t), identity cascades of
    1, 3 and 5 sections in each input form (the plan's win_t under a refused window, the generator under an accepted
    one) and two identity sections in f64 precision (d_win64, d_win_half).
    First MI355X run, worst of the 16 forms.  T1: 6.0e-8 against 2^-23 = 1.2e-7 (one rounding of x w), no nonzero sample at a
    zero, no wrong sign.  T2: 5.9e-8 of the peak against A(w) = 4.5e-7 on each of the five accepted windows (0.12 of the
    bound: 'time' applies the plan's table copy, one rounding).  T3: table windows 6.7e-7 against a float32-FFT bound of
    1.6e-6 (coded_zeros); generated windows 8.9e-7 against 1.9e-6 + 1.0e-6 (hann_in), Hann 5.8e-7."""
    fm = FORMS[form]
    xd, x64, kw = _input(torch_mod, fm)
    bad = []
    for window in fm.windows:
        w = _configure(ch, fm, window)
        out = _outputs(ch, xd, kw)
        generated = fm.gate == "T1/T2" and wc.VERDICTS[window]
        a, peak = wc.bound_of(window) if generated else (None, None)
        if not _mirror_ok(out):
            bad.append((window, "mag_full does not mirror mag_half"))
        if generated:
            ratio, frac = wc.gate_t2(out["time"], x64, w, a, peak)
            print(f"FIGURE window {form} {window} T2: worst {frac:.2e} of peak (A(w) {a:.2e}), error / bound {ratio:.2f}")
            if not ratio <= 1.0:
                bad.append((window, "T2", ratio, frac, a))
        else:
            fig = wc.gate_t1(out["time"], x64 * w)
            print(f"FIGURE window {form} {window} T1: time {fig[0]:.2e} (bound {2.0 ** -23:.2e}), nonzero at zeros {fig[1]}, "
                  f"wrong signs {fig[2]}")
            if not wc.t1_passes(fig):
                bad.append((window, "T1", fig))
        fig = wc.gate_t3(out["spec_half"][2:], out["mag_half"][2:], x64[2:], w, a, peak)
        print(f"FIGURE window {form} {window} T3: spec {fig[0]:.2e} mag {fig[1]:.2e} | float32-FFT bound {fig[2]:.2e} "
              f"+ window term {fig[3]:.2e}")
        if not wc.t3_passes(fig):
            bad.append((window, "T3", fig))
    assert not bad, bad


def _peak_rel(got, ref):
    return np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)


@pytest.mark.parametrize("form", [f for f, fm in FORMS.items() if fm.gate == "T4"])
def test_window_through_real_cascades(ch, torch_mod, oracle, form):
    """T4: mode 0x00 (the default plan's own window copy; reference: float64 sosfilt of the RTL taps), the unit-numerator
    cascades butter(12, 0.2), butter(8, 0.1) and butter(4, 0.002) (the gain folded into the window copy and into the
    generator) and butter(12, 0.2) in f64 precision, under `hamming` (generated in the float32 spectrum kernels) and
    `coded` (table): 'time' and spec_half of all four frames against float64 sosfilt + rfft of x w.  Bounds, per frame:
    time max(1e-5, 3 x a sequential float32 sosfilt) of the frame's peak (f64: 1e-6), spectrum in the bin norm
    max(1e-5, 3 x the sequential float32 spectrum) (f64: the float32-FFT bound).

    The window term.  Under a generated window the float32 spectrum kernels apply W, not the table w the reference is
    made with: a per-sample input error of at most A(w) peak |x_n| (include/specan.h), which the cascade passes with at
    most its peak gain max |H| and the transform spreads as in T3.  The spectrum bound of a generated window therefore
    carries the term A(w) peak |x|_2 max|H| / RMS_k |ref_k| -- T3's term behind the cascade.  It matters where the
    cascade removes the frame itself: the constant frames under Hamming through the RTL band-pass leave 1.5e-4 of their
    RMS, so a window error of 1.2e-7 of the peak is 1.4e-3 of that spectrum in exact arithmetic (float64 sosfilt + rfft
    of x W against x w; a sequential float32 sosfilt of x W gives 1.6e-3, the kernel 1.7e-3, a sequential float32
    sosfilt of x w 4.5e-4, three times which was the bound without the term).  On the noise and impulse frames the term
    is 3e-6 .. 4e-6, and `coded`, a table window, has none.
    First MI355X run.  mode 0x00: time 5.9e-6 (bound 1.8e-5), spectrum 1.7e-3 on the constant frames under Hamming (bound
    1.4e-3 + term 4.2e-3) and 2.8e-6 under coded (1e-5).  Unit forms: butter12 time 1.3e-6 (1e-5) spectrum 1.2e-5 (2.4e-5);
    butter8 2.8e-6 (1.5e-5) and 1.0e-4 (3.7e-4); long_memory 3.9e-5 (8.2e-3) and 6.0e-4 (2.7e-1).  f64 butter12: time
    4.2e-8 (1e-6), spectrum 9.2e-7 (3.2e-6)."""
    fm = FORMS[form]
    sos = wc.reference_sos(fm.cascade)
    xd, x64, kw = _input(torch_mod, fm)
    h_max = float(np.abs(signal.sosfreqz(sos, worN=8192)[1]).max())
    bad = []
    for window in fm.windows:
        w = _configure(ch, fm, window)
        out = _outputs(ch, xd, kw, ("time", "spec_half"))
        xw = x64 * w
        ref = signal.sosfilt(sos, xw, axis=1)
        R = np.fft.rfft(ref, axis=1)
        e_t = _peak_rel(out["time"].astype(np.float64), ref)
        e_s = np.array([sc.bin_norm(out["spec_half"][i], R[i]) for i in range(4)])
        if fm.precision == "f32":
            seq = np.stack([oracle.sosfilt_f32_c(sos, r) for r in xw.astype(np.float32)]).astype(np.float64)
            b_t = np.maximum(1e-5, 3 * _peak_rel(seq, ref))
            b_s = np.array([max(1e-5, 3 * sc.bin_norm(np.fft.rfft(seq[i]), R[i])) for i in range(4)])
            if wc.VERDICTS[window]:
                a, peak = wc.bound_of(window)
                term = a * peak * np.sqrt((x64 * x64).sum(axis=1)) * h_max / np.sqrt(np.mean(np.abs(R) ** 2, axis=1))
                print(f"FIGURE window {form} {window} T4: window term per frame {np.array2string(term, precision=2)}")
                b_s = b_s + term
        else:
            b_t = np.full(4, 1e-6)
            b_s = np.array([max(1e-6, sc.fft_bound(ref[i].astype(np.float32), R[i])) for i in range(4)])
        it, is_ = int(np.argmax(e_t / b_t)), int(np.argmax(e_s / b_s))
        print(f"FIGURE window {form} {window} T4: time {e_t[it]:.2e} (bound {b_t[it]:.2e}, {wc.FRAME_NAMES[it]}) "
              f"spectrum {e_s[is_]:.2e} (bound {b_s[is_]:.2e}, {wc.FRAME_NAMES[is_]})")
        if not ((e_t <= b_t).all() and (e_s <= b_s).all()):
            bad.append((window, e_t.tolist(), b_t.tolist(), e_s.tolist(), b_s.tolist()))
    assert not bad, bad


# --------------------------------------------------------------------------------------------------- T5: route independence
def _eq(torch, a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


def _run(ch, xd):
    return {k: ch.process_f32(xd, out_kind=k) for k in ("time", "mag_full")}


@pytest.mark.parametrize("cascade", ["butter12", "butter5_padded"])
@pytest.mark.parametrize("window", ["coded", "hamming"])
def test_every_route_reaches_the_state_of_a_fresh_handle(chain_cls, torch_mod, window, cascade):
    """T5: load_sos rebuilds the custom plan's window copy from the handle's window, set_window_f32 rebuilds both plans,
    entering f64 precision resynchronises the double tables.  Whatever the order of the control calls -- window then
    cascade, cascade then window, another window first, mode 0x00 entered before or after the window, f64 precision
    entered before the window, after it, or left, the window changed, and entered again -- 'time' and mag_full of modes
    0xA1 and 0x00 equal those of a fresh handle configured directly, bit for bit.  First MI355X run: every route equal."""
    torch = torch_mod
    w, other = wc.table(window), wc.table("coded_zeros" if window == "coded" else "cos_neg")
    sos = sc.cascades()[cascade]
    xd = to_device(torch, wc.frames(False)[0])

    def fresh(precision, mode):
        c = chain_cls(0)
        try:
            c.set_window_f32(w)
            c.load_sos(sos)
            c.set_filter_mode(mode)
            if precision == "f64":
                c.set_precision("f64")
            return _run(c, xd)
        finally:
            c.close()

    want = {(p, m): fresh(p, m) for p in ("f32", "f64") for m in (0xA1, 0x00)}
    assert not _eq(torch, want["f32", 0xA1], want["f32", 0x00])          # the two plans differ: the routes are told apart

    routes = {
        "cascade_then_window": [("sos",), ("mode", 0xA1), ("win", w)],
        "window_a_cascade_window_b": [("win", other), ("sos",), ("mode", 0xA1), ("win", w)],
        "mode00_then_window": [("mode", 0x00), ("win", w), ("check", 0x00), ("sos",), ("mode", 0xA1)],
        "window_then_mode00": [("win", w), ("mode", 0x00), ("check", 0x00), ("sos",), ("check", 0x00), ("mode", 0xA1)],
        "mode00_window_b_last": [("win", other), ("sos",), ("mode", 0xA1), ("run",), ("mode", 0x00), ("win", w),
                                 ("check", 0x00), ("mode", 0xA1)],
        "f64_before_window": [("prec", "f64"), ("win", w), ("sos",), ("mode", 0xA1)],
        "f64_after_window": [("win", w), ("sos",), ("mode", 0xA1), ("prec", "f64")],
        "f64_left_window_changed_reentered": [("win", other), ("sos",), ("mode", 0xA1), ("prec", "f64"), ("run",),
                                              ("prec", "f32"), ("win", w), ("check", 0xA1), ("prec", "f64")],
        "f64_cascade_changed_inside": [("prec", "f64"), ("win", w), ("mode", 0xA1), ("run",), ("sos",), ("check", 0xA1),
                                       ("prec", "f32")],
    }
    bad = []
    for name, steps in routes.items():
        c = chain_cls(0)
        try:
            def check(mode, where):
                if not _eq(torch, _run(c, xd), want[c.precision, mode]):
                    bad.append((name, where, c.precision, hex(mode)))

            for i, st in enumerate(steps):
                if st[0] == "win":
                    c.set_window_f32(st[1])
                elif st[0] == "sos":
                    c.load_sos(sos)
                elif st[0] == "mode":
                    c.set_filter_mode(st[1])
                elif st[0] == "prec":
                    c.set_precision(st[1])
                elif st[0] == "run":
                    _run(c, xd)
                else:
                    check(st[1], i)
            check(0xA1, "end")
            c.set_filter_mode(0x00)
            check(0x00, "end, mode 0x00")
        finally:
            c.close()
    print(f"FIGURE window routes {window} {cascade}: {len(routes)} routes, {len(bad)} differ from a fresh handle")
    assert not bad, bad


# ----------------------------------------------------------------------------------------------- T6: power-of-two windows
@pytest.mark.parametrize("mode", ["bypass", "butter12"])
@pytest.mark.parametrize("window", ["hamming", "coded", "hann_in"])
def test_power_of_two_window_scales_exactly(ch, torch_mod, window, mode):
    """T6: w 2^k, k = -20 and +20.  The fit is a linear solve on sums that scale exactly and its threshold is relative to
    the peak, so the verdict is that of w; every table made from the window scales exactly, so 'time' and spec_half are
    those of w times 2^k, bit for bit, in bypass mode and through butter(12, 0.2) in mode 0xA1 -- outside underflow:
    behind the impulse frame the cascade's response decays through the float32 denormals, where a value has fewer than
    24 bits and does not scale exactly (the first MI355X run differed there, in 'time' alone, by 1.4e-44 at k = -20, a few
    denormal steps, and by 2.4e-38 = 2^20 such steps at k = +20; spec_half was exact).  So a sample is compared bit for bit where both it and its scaled value are at least 2^-100,
    and within 2^-100 elsewhere; an exact zero is either way.
    First MI355X run: same verdict; exact for both k, every window and both modes on every sample of at least 2^-100."""
    fm = wc.Form(0xB1, None, "float32", None, "f32", (), "T1", 0, 0) if mode == "bypass" else FORMS["unit_butter12_f32"]
    xd, _, kw = _input(torch_mod, fm)
    _configure(ch, fm, window)
    base = _outputs(ch, xd, kw, ("time", "spec_half"))
    assert np.abs(base["time"]).max() > 0
    bad = []
    for k in (-20, 20):
        s = np.float32(2.0 ** k)
        _configure(ch, fm, window, scale=float(s))             # asserts the verdict (wingen) where a plan is launched
        ch.set_filter_mode(0xA1)
        assert sc.plan_header(ch.iir_plan())[2] == int(wc.VERDICTS[window])        # bypass forms too: the custom plan's flag
        ch.set_filter_mode(fm.mode)
        got = _outputs(ch, xd, kw, ("time", "spec_half"))
        for kind in got:
            want = base[kind] * s
            normal = np.minimum(np.abs(base[kind]), np.abs(want)) >= 2.0 ** -100
            differ = int(np.count_nonzero(got[kind][normal] != want[normal]))
            small = float(np.abs(got[kind] - want)[~normal].max(initial=0.0))
            print(f"FIGURE window pow2 {mode} {window} k={k} {kind}: {differ} samples differ of {int(normal.sum())} at or above "
                  f"2^-100; below it worst |difference| {small:.1e} (bound {2.0 ** -100:.1e})")
            if differ or not small <= 2.0 ** -100:
                bad.append((k, kind, differ, small))
    assert not bad, bad
