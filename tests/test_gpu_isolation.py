"""GPU: frame isolation.  A frame's outputs depend only on that frame and the control state of its call -- not on what a
workgroup that ran before it left in LDS, and not on a neighbour frame that holds NaN, Inf or overflows.

Every other GPU test feeds finite frames to a GPU that last ran finite data, so a kernel that reads an LDS word it did
not write (a stale word times a zero tap, a padded identity section, a skipped scan level, an unused side slot) and
cancels it arithmetically passes them all: 0 * x = 0 for finite garbage.  Here the garbage is NaN or Inf.

  - tests/hip/lds_fill.hip (built by the fixture below, loaded with ctypes; not part of the library) writes one 32-bit
    word to all 160 KiB of LDS of every CU, and probes, without writing, what a later dispatch finds there.
  - (a) float chain, (b) integer chain: lds_fill(P) then the call on the same stream.  The float chain must give the
    bits it gives after lds_fill(0), all finite; the integer chain the bits of the integer model (oracle.chain_q15).
    Victim batches are small enough that each of their workgroups is the first on its LDS slot.  Each test pins the set
    of kernel variants it launched, read from the handle's state (exported plan, precision, batch, input type).
  - (c) non-finite neighbours: every third frame of a batch holds a NaN, an Inf or overflows |X|^2; the other frames
    must be bit-identical to the same frames run as a clean-only batch, and finite.  Nothing is asserted about the bad
    frames except the shape of their rows.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import N, ROOT, load_golden
from gpu_support import ch, table_window, to_device, torch_mod  # noqa: F401 (fixtures)
from structured_cases import cascades, plan_header

HELPER_SRC = os.path.join(ROOT, "tests", "hip", "lds_fill.hip")
NAN_WORD = 0xFFFFFFFF          # NaN as float and as double; -1 as an int16 pair
INF_WORD = 0x7F800000          # +Inf as float
I16_MIN_WORD = 0x80008000      # -32768 as an int16 pair
FLOAT_POISON = (NAN_WORD, INF_WORD)
Q15_POISON = (NAN_WORD, INF_WORD, I16_MIN_WORD)
KINDS = ("mag_full", "mag_half", "spec_half", "time", "marker")
# out_kind runs of test (a): every kind, the marker over the full range and over a range inside the upper half
KIND_RUNS = (("mag_full", None), ("mag_half", None), ("spec_half", None), ("time", None), ("marker", (0, N)),
             ("marker", (9000, 12001)))
I16_SCALE = 1.0 / 2048


# ------------------------------------------------------------------------------------------------------ LDS helper
@pytest.fixture(scope="module")
def lds_helper_so(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    so = str(tmp_path_factory.mktemp("lds_fill") / "liblds_fill.so")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-fPIC", "-shared", HELPER_SRC, "-o", so],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return so


def test_lds_helper_cross_compiles(lds_helper_so):
    """CPU: the helper builds for gfx950 and exports its two C entry points."""
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    r = subprocess.run([nm, "-D", "--defined-only", lds_helper_so], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    text = {ln.split()[-1] for ln in r.stdout.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T"}
    assert {"lds_fill", "lds_probe"} <= text, r.stdout


class Lds:
    """lds_fill / lds_probe on the current torch stream, over a grid of 8 workgroups per CU."""

    def __init__(self, so, torch):
        self.torch = torch
        L = ctypes.CDLL(so)                    # torch is imported: the helper binds to the HIP runtime torch mapped
        L.lds_fill.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
        L.lds_probe.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        L.lds_fill.restype = L.lds_probe.restype = ctypes.c_int
        self.L = L
        self.grid = 8 * torch.cuda.get_device_properties(0).multi_processor_count
        self.counts = torch.empty(self.grid * 4, dtype=torch.int32, device="cuda")

    def _stream(self):
        return self.torch.cuda.current_stream().cuda_stream

    def fill(self, word):
        rc = self.L.lds_fill(word, self.grid, self._stream())
        assert rc == 0, f"lds_fill: hipError {rc}"

    def probe(self, word):
        """Words differing from `word`, one count per probe wave (-1 stays where a wave stored nothing)."""
        self.counts.fill_(-1)
        rc = self.L.lds_probe(word, self.grid, self.counts.data_ptr(), self._stream())
        assert rc == 0, f"lds_probe: hipError {rc}"
        return self.counts.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def lds(lds_helper_so, hip_lib_built, torch_mod):
    return Lds(lds_helper_so, torch_mod)


@pytest.mark.gpu
def test_lds_contents_survive_between_dispatches(lds, torch_mod):
    """The premise of the poisoning tests: what one dispatch writes to LDS is what the next dispatch on that CU reads.
    Fill, then probe with 8 workgroups per CU, each holding all 160 KiB: every probe wave must see the pattern in every
    word it reads.  The probe is not blind either: after filling one word, probing for another counts every word."""
    per_wave = 160 * 1024 // 4 // 4
    for word in (NAN_WORD, INF_WORD, I16_MIN_WORD, 0, 0x5A5A5A5A):
        torch_mod.cuda.synchronize()
        lds.fill(word)
        c = lds.probe(word)
        assert c.max() == 0, (
            f"LDS residue NOT observed for 0x{word:08X}: {np.count_nonzero(c)} of {c.size} probe waves saw other words "
            f"(worst {c.max()} of {per_wave}).  LDS does not reliably keep a dispatch's contents for the next one, so "
            f"every poisoning test in this module would pass vacuously.")
        c = lds.probe(word ^ 0x00010001)
        assert (c == per_wave).all(), (word, np.unique(c))
    print(f"FIGURE lds residue: {lds.grid} probe workgroups x 4 waves saw every fill pattern in all 160 KiB")


# ------------------------------------------------------------------------------------------------ frames, compare
def _frames_f32(B, seed):
    """Noise + a tone per frame; frame 0 an impulse, frame 1 all zero (any leaked NaN / Inf shows in its outputs)."""
    rng = np.random.default_rng(seed)
    n = np.arange(N)
    x = 0.3 * rng.standard_normal((B, N)) + 0.5 * np.sin(2 * np.pi * rng.uniform(0.01, 0.45, (B, 1)) * n)
    x[:2] = 0.0
    x[0, 0] = 1.0
    return x.astype(np.float32)


def _frames_i16(B, seed, amp=2048):
    rng = np.random.default_rng(seed)
    x = rng.integers(-amp, amp, (B, N))
    x[:2] = 0
    x[0, 0] = amp - 1
    if B > 2:
        x[-1] = rng.integers(-32768, 32768, N)            # one full-scale frame
    return x.astype(np.int16)


def _floats(kind, a):
    """The floating-point content of an output: marker records -> (peak_mag, band_power)."""
    return a.view(np.float32)[:, [0, 2]] if kind == "marker" else a


def _all_finite(kind, a):
    return bool(np.isfinite(_floats(kind, a)).all())


def _worst_delta(kind, a, b):
    """max |a - b| over the floating-point content (inf where a side is NaN or Inf and the bits differ); marker bins
    by their difference."""
    if _bits_equal(a, b):
        return 0.0
    fa, fb = np.ascontiguousarray(_floats(kind, a)), np.ascontiguousarray(_floats(kind, b))
    d = np.abs(fa.astype(np.complex128 if np.iscomplexobj(fa) else np.float64) - fb)
    w = float(np.where(np.isnan(d), np.inf, d).max())
    if kind == "marker":
        w = max(w, float(np.abs(a[:, 1].astype(np.int64) - b[:, 1]).max()))
    return w


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _after_fill(torch_mod, lds, word, call):
    """lds_fill(word), then `call` on the same stream, with nothing else in flight; the result on the host."""
    torch_mod.cuda.synchronize()
    lds.fill(word)
    return call().cpu().numpy()


# --------------------------------------------------------------------------------------- (a) float chain, poisoned
def _launched_f32(ch, x, kind):
    """(InT, nsec, unit, wingen, one_round, out_kind, precision) of the float kernel a process_f32 call launches, from
    the handle's state as specan_abi.cpp (process_float) and chain_f32.hpp (launch_chain) decide it.  The float64-state
    path launches iir_f64_kernel<nsec, InT> (window table, no unit form) and, unless out_kind is 'time', the bypassed
    chain on its float32 output."""
    in_t = str(x.dtype).replace("torch.", "")
    nsec = unit = wingen = 0
    if ch.filter_mode != 0xB1:
        nsec, unit, wingen, _ = plan_header(ch.iir_plan())
    if ch.precision == "f64" and nsec > 0:
        return (in_t, nsec, 0, 0, kind != "time" and x.shape[0] <= 512, kind, "f64")
    one_round = nsec == 0 and in_t == "float32" and kind != "time" and x.shape[0] <= 512
    return (in_t, nsec, unit, wingen if nsec else 0, one_round, kind, "f32")


def _variants(in_ts, nsec_unit, wingens, one_rounds, precision):
    """The tuples of _launched_f32 for every out kind; 'time' has no one-round form."""
    return {(t, ns, u, w, o and k != "time", k, precision)
            for t in in_ts for ns, u in nsec_unit for w in wingens for o in one_rounds for k in KINDS}


CASCADE_NSEC_UNIT = {(6, 1), (6, 0), (2, 1), (2, 0), (4, 0)}
F64_CASCADES = ("long_memory", "butter5_padded", "butter12", "rtl_default")     # padded nsec 2, 4, 6, 6

# group -> (configurations: (label, filter mode, cascade name or None, window, precision), inputs: (dtype, B), variants)
FLOAT_GROUPS = {
    "bypass": ([("bypass", 0xB1, None, "cos", "f32")],
               [("float32", 200), ("float32", 520), ("int16", 200), ("int16", 520)],
               _variants(("float32",), {(0, 0)}, (0,), (True, False), "f32")
               | _variants(("int16",), {(0, 0)}, (0,), (False,), "f32")),
    "defaults": ([("default_" + w, 0x00, None, w, "f32") for w in ("cos", "table")],
                 [("float32", 24), ("int16", 24)],
                 _variants(("float32", "int16"), {(6, 0)}, (0, 1), (False,), "f32")),
    "cascades_float32": ([(f"{n}_{w}", 0xA1, n, w, "f32") for n in cascades() for w in ("cos", "table")],
                         [("float32", 24)],
                         _variants(("float32",), CASCADE_NSEC_UNIT, (0, 1), (False,), "f32")),
    "cascades_int16": ([(f"{n}_{w}", 0xA1, n, w, "f32") for n in cascades() for w in ("cos", "table")],
                       [("int16", 24)],
                       _variants(("int16",), CASCADE_NSEC_UNIT, (0, 1), (False,), "f32")),
    "f64": ([(n + "_f64", 0xA1, n, "cos", "f64") for n in F64_CASCADES] + [("default_f64", 0x00, None, "cos", "f64")],
            [("float32", 24), ("int16", 24)],
            _variants(("float32", "int16"), {(2, 0), (4, 0), (6, 0)}, (0,), (True,), "f64")),
}


def _configure(ch, mode, casc, window, precision):
    ch.set_precision("f32")
    ch.set_window_f32(None if window == "cos" else table_window())
    if casc == "smoother_f32":
        ch.load_sos_f32(cascades()[casc])
    elif casc is not None:
        ch.load_sos(cascades()[casc])
    ch.set_filter_mode(mode)
    ch.set_precision(precision)


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(FLOAT_GROUPS))
def test_poisoned_lds_float_chain(ch, torch_mod, lds, group):
    """(a) lds_fill(P) then process_f32, for P = NaN / +Inf words, against the same call after lds_fill(0): bit for bit,
    and every output finite.  Every out kind (the marker over the full range and over [9000, 12001)); the group's
    configurations and batches reach exactly the variant set the group pins (see FLOAT_GROUPS)."""
    configs, inputs, want = FLOAT_GROUPS[group]
    reached, bad, worst, n_calls = set(), [], 0.0, 0
    for label, mode, casc, window, precision in configs:
        _configure(ch, mode, casc, window, precision)
        for in_t, B in inputs:
            x = _frames_f32(B, B) if in_t == "float32" else _frames_i16(B, B)
            xd = to_device(torch_mod, x)
            kw = {"scale": I16_SCALE} if in_t == "int16" else {}
            for kind, rng in KIND_RUNS:
                if rng is not None:
                    ch.set_marker_range(*rng)
                reached.add(_launched_f32(ch, xd, kind))
                call = lambda: ch.process_f32(xd, out_kind=kind, **kw)     # noqa: E731
                ref = _after_fill(torch_mod, lds, 0, call)
                if not _all_finite(kind, ref):
                    bad.append((label, in_t, B, kind, rng, "after fill 0", "non-finite"))
                for word in FLOAT_POISON:
                    got = _after_fill(torch_mod, lds, word, call)
                    n_calls += 1
                    d = _worst_delta(kind, got, ref)
                    worst = max(worst, d)
                    if not _bits_equal(got, ref) or not _all_finite(kind, got):
                        rows = int(np.count_nonzero((got != ref).reshape(B, -1).any(axis=1)))
                        bad.append((label, in_t, B, kind, rng, f"0x{word:08X}", f"{rows} rows differ, worst |d| {d:.3g}",
                                    "finite" if _all_finite(kind, got) else "NON-FINITE"))
    ch.set_marker_range(0, N)
    print(f"FIGURE poisoned float {group}: {n_calls} poisoned calls, {len(reached)} variants, worst |d| {worst:.3g}")
    assert not bad, "\n".join(map(str, bad[:10]))
    assert reached == want, (sorted(want - reached), sorted(reached - want))


def test_float_poison_groups_cover_every_form():
    """CPU: the union of the variant sets pinned by test_poisoned_lds_float_chain covers both input types, padded
    section counts 0/2/4/6, both numerator forms, both window forms, the one- and two-round bypass, every out kind and
    both precisions, and the float64-state path at nsec 2, 4 and 6 on both inputs."""
    allv = set().union(*(g[2] for g in FLOAT_GROUPS.values()))
    assert {v[0] for v in allv} == {"float32", "int16"}
    assert {v[1] for v in allv} == {0, 2, 4, 6}
    assert {v[2] for v in allv if v[6] == "f32" and v[1]} == {0, 1}
    assert {v[3] for v in allv if v[6] == "f32" and v[1]} == {0, 1}
    assert {v[4] for v in allv if v[0] == "float32" and v[1] == 0} == {True, False}
    assert {v[5] for v in allv} == set(KINDS)
    assert {(v[0], v[1]) for v in allv if v[6] == "f64"} == {(t, n) for t in ("float32", "int16") for n in (2, 4, 6)}


# ------------------------------------------------------------------------------------- (b) integer chain, poisoned
C12_B1 = np.array([0, 1, 0, 64, -67, 19, 64, 127, 64, 64, -85, 40], np.int8)          # B1 != 0: the long step
C12_NOB1 = np.array([32, 0, -32, 64, -67, 19, 64, 0, 64, 64, -85, 40], np.int8)       # B1 = 0 in both sets

# label -> (filter mode, Q7 upload, Q2.14 sections, kernels of filter_q15, kernels of process_q15)
Q15_CASES = {
    "bypass": (0xB1, None, 0, ("window_q15",), ("fft_q15<true>",)),
    "default": (0x00, None, 0, ("filter_q7<true>",), ("filter_q7<true>", "fft_q15<false>")),
    "custom_nob1": (0xA1, C12_NOB1, 0, ("filter_q7<true>",), ("filter_q7<true>", "fft_q15<false>")),
    "custom_b1": (0xA1, C12_B1, 0, ("filter_q7<false>",), ("filter_q7<false>", "fft_q15<false>")),
    "wide1": (0xA2, None, 1, ("filter_w14/1",), ("filter_w14/1", "fft_q15<false>")),
    "wide3": (0xA2, None, 3, ("filter_w14/3",), ("filter_w14/3", "fft_q15<false>")),
    "wide6": (0xA2, None, 6, ("filter_w14/6",), ("filter_w14/6", "fft_q15<false>")),
}


def _launched_q15(ch, nsec_wide, fft):
    """The kernels a Q15 call launches, from the handle's state as specan_abi.cpp (process_q15) and cascade_q15.hip
    (sa_launch_filter_q15: the short step when B1 = 0 in both coefficient sets; 0x00 runs the fixed taps, whose B1 is 0)."""
    mode = ch.filter_mode
    if mode == 0xB1:
        return ("fft_q15<true>",) if fft else ("window_q15",)
    if mode == 0xA2:
        filt = f"filter_w14/{nsec_wide}"
    else:
        c = ch.coeffs_q7()
        filt = f"filter_q7<{'true' if mode == 0x00 or (c[1] == 0 and c[7] == 0) else 'false'}>"
    return (filt, "fft_q15<false>") if fft else (filt,)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(Q15_CASES))
def test_poisoned_lds_integer_chain(ch, torch_mod, oracle, lds, case):
    """(b) lds_fill(P) then filter_q15 / process_q15, for P = NaN / +Inf / (-32768, -32768) words: bit for bit the
    integer model, in both window modes, at ragged batches 1, 7 and 17 (the last workgroup of the cascade kernels has
    idle frame pairs, which still take part in the barriers)."""
    mode, c12, nsec_wide, want_filt, want_fft = Q15_CASES[case]
    sos14 = load_golden("g4_q15_frames.npz")["sos_q14"][:max(1, nsec_wide)]
    if c12 is not None:
        ch.load_coeffs_q7(c12)
    if nsec_wide:
        ch.load_sos_q14(sos14)
    ch.set_filter_mode(mode)
    reached, bad, n_calls = set(), [], 0
    for win_mode in (0, 1):
        ch.set_window_mode_q15(win_mode)
        for B in (1, 7, 17):
            x = _frames_i16(B, 100 * B + win_mode, amp=8192)
            ref_iq, ref_t = oracle.chain_q15(x, None, win_mode, mode, c12, sos14 if nsec_wide else None, want_time=True)
            xd = to_device(torch_mod, x)
            reached.add((_launched_q15(ch, nsec_wide, False), win_mode))
            reached.add((_launched_q15(ch, nsec_wide, True), win_mode))
            for word in Q15_POISON:
                t = _after_fill(torch_mod, lds, word, lambda: ch.filter_q15(xd))
                iq = _after_fill(torch_mod, lds, word, lambda: ch.process_q15(xd))
                n_calls += 2
                for what, got, ref in (("filter_q15", t, ref_t), ("process_q15", iq, ref_iq)):
                    if not np.array_equal(got, ref):
                        rows = np.flatnonzero((got != ref).reshape(B, -1).any(axis=1)).tolist()
                        bad.append((case, win_mode, B, f"0x{word:08X}", what, "rows", rows))
    print(f"FIGURE poisoned q15 {case}: {n_calls} poisoned calls bit-exact: {sorted(reached)}")
    assert not bad, "\n".join(map(str, bad[:10]))
    assert reached == {(k, w) for k in (want_filt, want_fft) for w in (0, 1)}


# --------------------------------------------------------------------------------- (c) non-finite neighbour frames
BAD_F32 = ("nan_sample", "pos_inf_sample", "neg_inf_sample", "all_nan", "overflow_1e30")


def _spoil_f32(x, i, what, rng):
    j = int(rng.integers(0, N))
    if what == "nan_sample":
        x[i, j] = np.nan
    elif what == "pos_inf_sample":
        x[i, j] = np.inf
    elif what == "neg_inf_sample":
        x[i, j] = -np.inf
    elif what == "all_nan":
        x[i] = np.nan
    else:
        x[i] = (1e30 * rng.standard_normal(N)).astype(np.float32)     # finite; |X|^2 overflows float32


def _mixed_f32(B, seed, bad_of_3=1):
    """B frames of which `bad_of_3` in every 3 are bad (cycling through BAD_F32): (batch, indices of the clean ones)."""
    rng = np.random.default_rng(seed)
    x = _frames_f32(B, seed)
    bad_idx = [i for i in range(B) if i % 3 >= 3 - bad_of_3]
    for k, i in enumerate(bad_idx):
        _spoil_f32(x, i, BAD_F32[k % len(BAD_F32)], rng)
    return x, np.array([i for i in range(B) if i % 3 < 3 - bad_of_3])


I16_BIG_SCALE = 2.0 ** 40      # clean frames (|sample| <= 8) stay finite; full-scale frames overflow |X|^2 in float32


def _mixed_i16(B, seed):
    """Every third frame full scale (a constant, a tone at bin 4096, random): |X|^2 overflows at I16_BIG_SCALE in
    every filter mode (the default cascade stops DC, so the tone; the low-pass cascade passes DC)."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-8, 9, (B, N)).astype(np.int16)
    bad_idx = list(range(2, B, 3))
    n = np.arange(N)
    for k, i in enumerate(bad_idx):
        x[i] = (32767, np.rint(32767 * np.cos(2 * np.pi * 4096 * n / N)), rng.integers(-32768, 32768, N))[k % 3]
    return x, np.array([i for i in range(B) if i % 3 != 2])


# label -> (filter mode, cascade name, precision).  Precision does not apply in mode 0xB1 (include/specan.h): the
# float64 bypass would be the same launch as the float32 one, so it is not repeated.
NEIGHBOUR_FORMS = {
    "bypass": (0xB1, None, "f32"),
    "default": (0x00, None, "f32"),
    "default_f64": (0x00, None, "f64"),
    "custom6": (0xA1, "butter12", "f32"),
    "custom6_f64": (0xA1, "butter12", "f64"),
}


def _check_neighbours(ch, torch_mod, x, clean, kinds, tag, **kw):
    xd = to_device(torch_mod, x)
    cd = to_device(torch_mod, x[clean])
    bad, spoilt = [], 0
    for kind in kinds:
        mixed = ch.process_f32(xd, out_kind=kind, **kw).cpu().numpy()
        ref = ch.process_f32(cd, out_kind=kind, **kw).cpu().numpy()
        got = mixed[clean]
        assert mixed.shape[0] == x.shape[0]
        if not _all_finite(kind, ref):
            bad.append((tag, kind, "clean-only batch non-finite"))
        if not _bits_equal(got, ref) or not _all_finite(kind, got):
            rows = np.flatnonzero((got != ref).reshape(len(clean), -1).any(axis=1))
            bad.append((tag, kind, f"{rows.size} clean rows differ, e.g. frames {clean[rows[:5]].tolist()}, "
                                   f"worst |d| {_worst_delta(kind, got, ref):.3g}"))
        rest = np.setdiff1d(np.arange(x.shape[0]), clean)
        spoilt += int((~np.isfinite(_floats(kind, mixed[rest]).reshape(len(rest), -1))).any(axis=1).sum())
    return bad, spoilt


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(NEIGHBOUR_FORMS))
def test_nonfinite_neighbour_frames(ch, torch_mod, form):
    """(c) float32 batches of 1024 (two-round bypass; later workgroups inherit LDS from bad ones) and 300 (one-round
    bypass) where every third frame holds one NaN, +Inf or -Inf sample, is all NaN, or has magnitude 1e30: the clean
    frames equal, bit for bit, the same frames run as a clean-only batch, and are finite, for every out kind."""
    mode, casc, precision = NEIGHBOUR_FORMS[form]
    _configure(ch, mode, casc, "cos", precision)
    bad, spoilt = [], 0
    for B in (1024, 300):
        x, clean = _mixed_f32(B, B)
        b, s = _check_neighbours(ch, torch_mod, x, clean, KINDS, (form, B))
        bad += b
        spoilt += s
    print(f"FIGURE neighbours {form}: clean frames bit-identical; {spoilt} bad rows with non-finite outputs (not asserted)")
    assert not bad, "\n".join(map(str, bad))


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(NEIGHBOUR_FORMS))
def test_nonfinite_neighbour_frames_int16(ch, torch_mod, form):
    """(c) the int16 entry at scale 2^40, where a full-scale frame overflows |X|^2 in float32: the clean frames
    (|sample| <= 8) equal the clean-only batch bit for bit and are finite, for every out kind."""
    mode, casc, precision = NEIGHBOUR_FORMS[form]
    _configure(ch, mode, casc, "cos", precision)
    x, clean = _mixed_i16(1024, 7)
    bad, spoilt = _check_neighbours(ch, torch_mod, x, clean, KINDS, (form, "int16"), scale=I16_BIG_SCALE)
    print(f"FIGURE neighbours int16 {form}: clean frames bit-identical; {spoilt} bad rows with non-finite outputs "
          f"(not asserted)")
    assert spoilt > 0, "no full-scale frame overflowed: the scale no longer tests overflow"
    assert not bad, "\n".join(map(str, bad))


@pytest.mark.gpu
def test_nonfinite_neighbours_overlapped(ch, torch_mod):
    """(c) at overlap depth 2: a bad-heavy call (two frames in three bad) alternates with a clean call so that the two
    run side by side; after flush() the clean call and the clean frames of the bad-heavy call equal the stream-ordered
    results bit for bit, for every out kind."""
    _configure(ch, 0x00, None, "cos", "f32")
    xb, clean_b = _mixed_f32(1024, 11, bad_of_3=2)
    xc = _frames_f32(1024, 12)
    db, dc = to_device(torch_mod, xb), to_device(torch_mod, xc)
    ref_b = {k: ch.process_f32(db, out_kind=k).cpu().numpy()[clean_b] for k in KINDS}
    ref_c = {k: ch.process_f32(dc, out_kind=k).cpu().numpy() for k in KINDS}
    ch.set_overlap(2)
    outs = []
    for k in KINDS:
        for _ in range(2):
            outs.append((k, "bad-heavy", ch.process_f32(db, out_kind=k)))
            outs.append((k, "clean", ch.process_f32(dc, out_kind=k)))
    ch.flush()
    bad = []
    for k, which, o in outs:
        got = o.cpu().numpy()
        got, ref = (got[clean_b], ref_b[k]) if which == "bad-heavy" else (got, ref_c[k])
        if not _bits_equal(got, ref) or not _all_finite(k, got):
            bad.append((k, which, _worst_delta(k, got, ref)))
    ch.set_overlap(1)
    assert not bad, "\n".join(map(str, bad))
