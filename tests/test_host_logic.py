"""CPU: host-side logic -- designer/quantiser mirror, frame helpers, IIR plan algebra."""
import ctypes

import numpy as np
import pytest

from udp_collect import FrameCollector
from conftest import N, load_golden, rel_maxnorm
from fpga_real_time_fft_analyzer_amd import designer, frames


# ---- IIR-4: designer + quantiser against the reference's outputs (G5)
@pytest.mark.parametrize("kind", ["butter", "cheby1", "cheby2", "ellip", "bessel"])
def test_designer_and_quantiser_match_reference(kind):
    g = load_golden("g5_quantiser.npz")
    sos = designer.design_iir_filter("lowpass", 4, 10.0, 20.0, 100.0, kind=kind, ripple=1.0, attenuation=40)
    assert np.allclose(sos, g[f"sos_{kind}"], rtol=1e-12, atol=0)
    q = np.array(designer.quantize_coefficients(sos), dtype=np.int8)
    assert np.array_equal(q, g[f"q_{kind}"])


@pytest.mark.parametrize("ft", ["highpass", "bandpass", "bandstop"])
def test_designer_filter_types(ft):
    g = load_golden("g5_quantiser.npz")
    sos = designer.design_iir_filter(ft, 4, 10.0, 20.0, 100.0, kind="butter")
    assert np.allclose(sos, g[f"sos_butter_{ft}"], rtol=1e-12)
    assert np.array_equal(np.array(designer.quantize_coefficients(sos), np.int8), g[f"q_butter_{ft}"])


def test_designer_defaults_and_errors():
    g = load_golden("g5_quantiser.npz")
    q = designer.quantize_coefficients(designer.design_iir_filter("lowpass", 4, 10.0, 20.0, 100.0))
    assert np.array(q).tolist() == [[0, 1, 0, 64, -67, 19], [64, 127, 64, 64, -85, 40]]     # SURVEY IIR-4
    q12 = np.array(designer.quantize_coefficients(designer.design_iir_filter("lowpass", 12, 10.0, None, 100.0)))
    assert np.array_equal(q12, g["q_butter12"]) and q12[0].tolist() == [0, 0, 0, 64, -65, 17]
    with pytest.raises(ValueError):
        designer.design_iir_filter("lowpass", 4, 10.0, kind="fir")
    # band types default cutoff2 = 2*cutoff (gui.py:134-135)
    a = designer.design_iir_filter("bandpass", 2, 10.0, None, 100.0)
    b = designer.design_iir_filter("bandpass", 2, 10.0, 20.0, 100.0)
    assert np.array_equal(a, b)


def test_upload_bytes_and_padding():
    q = designer.quantize_coefficients(designer.design_iir_filter("lowpass", 2, 10.0, 20.0, 100.0))
    secs = designer.two_sections_for_fpga(q)
    assert len(secs) == 2 and secs[1] == [64, 0, 0, 64, 0, 0]             # gui.py:1190
    q12 = designer.quantize_coefficients(designer.design_iir_filter("lowpass", 12, 10.0, 20.0, 100.0))
    assert len(designer.two_sections_for_fpga(q12)) == 2                     # gui.py:1186-1187 truncation
    b = designer.coefficient_upload_bytes([[0, 1, 0, 64, -67, 19], [64, 127, 64, 64, -85, 40]])
    assert b == bytes([0xF1, 0, 1, 0, 64, 0xBD, 19, 64, 127, 64, 64, 0xAB, 40])
    assert designer.int8_to_byte(-1) == 255 and designer.int8_to_byte(127) == 127


def test_response_preview_tracks_the_integer_cascade(oracle):
    """N4: the small-signal response of the uploaded bytes (RTL port mapping, two sections x 3) must
    describe what the integer cascade does: a large-amplitude tone through the bit-exact model comes out
    with the previewed gain (truncation noise is a few LSB per section)."""
    from scipy import signal
    default = [[-14, 0, 14, 107, 21, 0], [-15, 0, 15, 107, -21, 0]]          # filter_pkg.vhd:54-68
    sos_eff = designer.fpga_effective_sos(default)
    assert sos_eff.shape == (6, 6) and np.array_equal(sos_eff[0], sos_eff[2]) and np.array_equal(sos_eff[1], sos_eff[5])
    assert sos_eff[0].tolist() == [14 / 128, 0.0, -14 / 128, 1.0, 21 / 128, 107 / 128]
    n = np.arange(N)
    for k in (3900, 4096, 4300):                                               # inside the pass band near fs/4
        x = np.rint(12000 * np.sin(2 * np.pi * k * n / N)).astype(np.int16)
        y = oracle.iir12_q7(x, np.array(default, np.int8).reshape(-1))
        y_lin = signal.sosfilt(sos_eff, x.astype(np.float64))
        assert np.max(np.abs(y[2048:] - y_lin[2048:])) <= 0.02 * np.max(np.abs(y_lin)) + 24
    w, h = designer.quantised_response(default, fs=1000.0, worN=4096)
    assert w[np.argmax(np.abs(h))] == pytest.approx(250.0, abs=15.0)           # band-pass near fs/4 (SURVEY IIR-3)
    w2, h2 = designer.filter_response(designer.design_iir_filter("lowpass", 4, 10.0, 20.0, 100.0))
    assert len(w2) == 2048 and abs(h2[0]) == pytest.approx(1.0, rel=1e-9)      # gui.py:193 worN
    url = designer.generate_filter_response_plot(designer.design_iir_filter("lowpass", 4, 10.0, 20.0, 100.0), 100.0,
                                                 quantized_two_sections=[[0, 1, 0, 64, -67, 19], [64, 127, 64, 64, -85, 40]])
    assert url is None or url.startswith("data:image/png;base64,")


def test_q14_quantiser(oracle):
    sos = load_golden("g2_config1.npz")["sos"]
    assert np.array_equal(designer.quantize_sos_q14(sos), oracle.quantize_sos_q14(sos))
    assert np.array_equal(designer.quantize_sos_q14(sos), load_golden("g4_q15_frames.npz")["sos_q14"])


# ---- OUT-1: frame helpers against the reference decoder's output (G6)
def test_frame_helpers():
    g = load_golden("g6_frame.npz")
    frame = g["frame"].tobytes()
    assert np.array_equal(frames.decode_mag_16iq_le(frame), g["mag"])
    re, im = frames.decode_iq_components(frame)
    assert np.array_equal(re, g["re"]) and np.array_equal(im, g["im"])
    with pytest.raises(ValueError):
        frames.decode_mag_16iq_le(frame[:-1])
    assert frames.frequency_axis_khz()[1] == pytest.approx(1e6 / 16384 / 1e3)


def test_udp_packetiser_roundtrip():
    g = load_golden("g6_frame.npz")
    frame = g["frame"].tobytes()
    pk = frames.frame_to_udp_payloads(frame)
    assert len(pk) == 64 and all(len(p) == 1025 for p in pk) and [p[0] for p in pk] == list(range(64))
    asm = FrameCollector()
    order = list(range(64))
    np.random.default_rng(3).shuffle(order)
    got = None
    for i in order:
        assert got is None
        got = asm.add(pk[i], 0)
    assert got == frame and asm.frames == 1
    assert asm.add(b"\x40" + bytes(1024), 0) is None          # index out of range ignored
    assert asm.add(bytes(10), 0) is None                      # wrong length ignored
    assert asm.add(pk[0], 0) is None and asm.frames == 1      # a partial frame stays pending (the collector has no time-out)


def test_pack_frame_is_little_endian(hip_lib_built):
    from fpga_real_time_fft_analyzer_amd.chain import pack_frame
    g = load_golden("g6_frame.npz")
    iq = np.frombuffer(g["frame"].tobytes(), "<i2").reshape(N, 2)
    assert pack_frame(iq) == g["frame"].tobytes()


# ---- IIR plan algebra: emulate the kernel's predict / scan / recurse in float32 on the CPU
def _parse_plan(plan):
    """Flat view written by sa_iir_plan_from_sos: SaIirK (nsec, unit, gain, pad, 6 x {c[8], pc[4], mback[4],
    plev[4][4], prow[4][4]}) followed by the predictor taps m[6][16][2], their half-chunk matrices p16[6][4] (A^16) and
    SaIirLaneTab's p[6][16][4].  Taps and matrices are in the section's pole coordinates; mback takes a state back to
    DF2T."""
    nsec = int(plan[:1].view(np.int32)[0])
    unit = int(plan[1:2].view(np.int32)[0])
    gain = float(plan[2]) if unit else 1.0
    off, secs = 4, []
    for _ in range(6):
        c = plan[off:off + 8]; off += 8        # b0,b1,b2,a1,a2, flags (int), pad, pad
        pc = plan[off:off + 4]; off += 4
        mback = plan[off:off + 4]; off += 4
        plev = plan[off:off + 16].reshape(4, 4); off += 16
        prow = plan[off:off + 16].reshape(4, 4); off += 16
        secs.append([c, pc, plev, prow, None, mback])
    mt = plan[off:off + 6 * 32].reshape(6, 16, 2); off += 6 * 32
    p16 = plan[off:off + 6 * 4].reshape(6, 4); off += 6 * 4
    for i in range(6):
        secs[i][4] = (mt[i], p16[i])
    lt = plan[off:off + 6 * 64].reshape(6, 16, 4); off += 6 * 64
    assert off == plan.size
    return nsec, secs, lt, np.float32(gain)


def _ks(z, mats):
    """4-level Kogge-Stone affine scan along axis -2 (16 entries), zero fill, float32."""
    f = np.float32
    for lev, d in enumerate((1, 2, 4, 8)):
        p = mats[lev]
        u = np.zeros_like(z)
        u[..., d:, :] = z[..., :-d, :]
        z = np.stack([(z[..., 0] + (p[0] * u[..., 0] + p[1] * u[..., 1])).astype(f),
                      (z[..., 1] + (p[2] * u[..., 0] + p[3] * u[..., 1])).astype(f)], axis=-1)
    return z


def emulate_chunked_iir(plan, x):
    """float32 emulation with the kernel's structure: thread t owns samples [64t, 64t+64) as chunks
    A,B of 32; per section: predict -> in-row scan (16 threads) -> scan over the 16 row totals ->
    start states -> DF2T recursion on both chunks."""
    f = np.float32
    nsec, secs, lt, gain = _parse_plan(plan)
    v = (x.astype(f) * gain).astype(f).reshape(256, 2, 32).copy()   # unit form: cascade gain folded into the window              # [thread][chunk][j]
    for s in range(nsec):
        c, pc, plev, prow, m, mb = secs[s]
        m, p16 = m
        z = np.zeros((256, 2, 2), f)                         # [thread][chunk][state]
        for hh in range(2):                                  # block Horner over the two half chunks (predict_chunk_ends)
            for j in range(16):
                z[:, :, 0] += m[j, 0] * v[:, :, 16 * hh + j]
                z[:, :, 1] += m[j, 1] * v[:, :, 16 * hh + j]
            if hh == 0:
                z = np.stack([p16[0] * z[..., 0] + p16[1] * z[..., 1], p16[2] * z[..., 0] + p16[3] * z[..., 1]], axis=-1).astype(f)
        zA, zB = z[:, 0, :], z[:, 1, :]
        zT = np.stack([pc[0] * zA[:, 0] + pc[1] * zA[:, 1] + zB[:, 0],
                       pc[2] * zA[:, 0] + pc[3] * zA[:, 1] + zB[:, 1]], axis=-1).astype(f)
        inc = _ks(zT.reshape(16, 16, 2), plev)               # [row][lane][state]
        exc = np.zeros_like(inc)
        exc[:, 1:, :] = inc[:, :-1, :]
        rows = _ks(inc[:, 15, :].reshape(1, 16, 2), prow)[0]  # inclusive over rows
        C = np.zeros((16, 2), f)
        C[1:] = rows[:-1]
        lp = lt[s]                                            # [16][4]
        sA = np.stack([exc[..., 0] + lp[None, :, 0] * C[:, None, 0] + lp[None, :, 1] * C[:, None, 1],
                       exc[..., 1] + lp[None, :, 2] * C[:, None, 0] + lp[None, :, 3] * C[:, None, 1]],
                      axis=-1).astype(f).reshape(256, 2)
        sB = np.stack([pc[0] * sA[:, 0] + pc[1] * sA[:, 1] + zA[:, 0],
                       pc[2] * sA[:, 0] + pc[3] * sA[:, 1] + zA[:, 1]], axis=-1).astype(f)
        back = lambda q: np.stack([mb[0] * q[:, 0] + mb[1] * q[:, 1], mb[2] * q[:, 0] + mb[3] * q[:, 1]], axis=-1).astype(f)
        sA, sB = back(sA), back(sB)                           # pole coordinates -> DF2T states
        s1 = np.stack([sA[:, 0], sB[:, 0]], axis=1)           # [thread][chunk]
        s2 = np.stack([sA[:, 1], sB[:, 1]], axis=1)
        b0, b1, b2, a1, a2 = c[:5]
        for j in range(32):
            xx = v[:, :, j]
            y = (b0 * xx + s1).astype(f)
            s1 = (b1 * xx + s2 - a1 * y).astype(f)
            s2 = (b2 * xx - a2 * y).astype(f)
            v[:, :, j] = y
    return v.reshape(-1)


def test_scan_in_pole_coordinates_keeps_sequential_accuracy(hip_lib_built, oracle):
    """Poles close to the real axis (pole angle 0.008 rad here) make the powers of the DF2T transition matrix
    grow to ~1/angle; with the scan run in DF2T coordinates the float32 result of this cascade was 28x worse
    than a sequential float32 sosfilt (1.6e-3 against 5.8e-5 of max|y|).  The plan keeps taps and scan
    matrices in pole coordinates: the emulation of the kernel's algebra must stay within 3x of sequential."""
    from scipy.signal import sosfilt
    from fpga_real_time_fft_analyzer_amd.chain import iir_plan_from_sos
    sos = np.array([[1.31712426e-03, -9.33410745e-04, 1.31712426e-03, 1.0, 1.91684936e+00, 9.20172522e-01],
                    [1.0, -1.69525561e+00, 1.0, 1.0, -1.98349975e+00, 9.83634833e-01]])     # cheby2 band-stop, order 2
    plan = iir_plan_from_sos(sos)
    rng = np.random.default_rng(2)
    n = np.arange(N)
    x = (0.6 * np.sin(2 * np.pi * 0.0127 * n) + 0.1 * rng.standard_normal(N)).astype(np.float32)
    xw = (x * oracle.hann_f64().astype(np.float32) * np.float32(0.5)).astype(np.float32)
    ref = sosfilt(sos, xw.astype(np.float64))
    seq = oracle.sosfilt_f32_c(sos, xw)
    e_seq = np.abs(seq - ref).max() / np.abs(ref).max()
    e_chunked = np.abs(emulate_chunked_iir(plan, xw) - ref).max() / np.abs(ref).max()
    assert e_chunked <= 3 * e_seq, (e_chunked, e_seq)
    # the back-transform is the identity for first-order and padding sections
    _, secs, _, _ = _parse_plan(iir_plan_from_sos(np.array([[0.2, 0.2, 0.0, 1.0, -0.6, 0.0]])))
    assert all(np.array_equal(sec[5], [1, 0, 0, 1]) for sec in secs[:2])


def test_iir_plan_reproduces_sosfilt(hip_lib_built, oracle):
    from scipy.signal import sosfilt
    from fpga_real_time_fft_analyzer_amd.chain import iir_plan_from_sos
    g = load_golden("g3_fp32_frames.npz")
    sos = g["sos"]
    plan = iir_plan_from_sos(sos)
    assert plan.size == 4 + 6 * (8 + 4 + 4 + 16 + 16 + 32 + 4) + 6 * 16 * 4
    hann = oracle.hann_f64()
    for i in range(2):
        xw = (g["x"][i].astype(np.float64) * hann).astype(np.float32)
        ref = sosfilt(sos, xw.astype(np.float64))
        y = emulate_chunked_iir(plan, xw)
        assert rel_maxnorm(y[None, :], ref[None, :]) <= 1e-5
    # the Butterworth cascade is eligible for the unit-numerator form (b2 == b0 in every section) ...
    assert int(plan[1:2].view(np.int32)[0]) == 1 and abs(float(plan[2]) - np.prod(sos[:, 0])) <= 1e-6 * np.prod(sos[:, 0])
    # ... the RTL default taps (b2 = -b0) or a padded 3-section cascade are not, and take the general path
    rtl = np.array([[14 / 128, 0, -14 / 128, 1, 21 / 128, 107 / 128], [15 / 128, 0, -15 / 128, 1, -21 / 128, 107 / 128]])
    for other in (rtl, sos[:3]):
        p2 = iir_plan_from_sos(other)
        assert int(p2[1:2].view(np.int32)[0]) == 0
        xw = (g["x"][0].astype(np.float64) * hann).astype(np.float32)
        assert rel_maxnorm(emulate_chunked_iir(p2, xw)[None, :], sosfilt(other, xw.astype(np.float64))[None, :]) <= 1e-5


def test_iir_plan_rejects_bad_sos(hip_lib_built):
    from fpga_real_time_fft_analyzer_amd.abi import SpecanError
    from fpga_real_time_fft_analyzer_amd.chain import iir_plan_from_sos
    with pytest.raises(SpecanError):
        iir_plan_from_sos(np.zeros((7, 6)))
    with pytest.raises(SpecanError):
        iir_plan_from_sos(np.array([[1, 0, 0, 0, 0, 0.0]]))     # a0 = 0
    assert int(iir_plan_from_sos(np.zeros((0, 6)))[:1].view(np.int32)[0]) == 0


# ---- the tables of chain.py that every process call goes through (no handle, no GPU)
def _chains():
    from fpga_real_time_fft_analyzer_amd.chain import FLOAT_CHAIN, Q15_CHAIN, Q15_WINDOW_CHAIN
    return {"float": FLOAT_CHAIN, "q15": Q15_CHAIN, "window": Q15_WINDOW_CHAIN}


def test_output_spec_table():
    import torch
    from fpga_real_time_fft_analyzer_amd.abi import SA_EINVAL, SpecanError
    from fpga_real_time_fft_analyzer_amd.chain import output_spec
    chains = _chains()
    want = {("float", "mag_full"): ((N,), torch.float32), ("float", "time"): ((N,), torch.float32),
            ("float", "mag_half"): ((8193,), torch.float32), ("float", "spec_half"): ((8193,), torch.complex64),
            ("float", "marker"): ((4,), torch.int32),
            ("q15", "iq"): ((N, 2), torch.int16), ("q15", "mag"): ((N,), torch.float32),
            ("q15", "marker"): ((4,), torch.int32),
            ("window", None): ((N,), torch.int16)}
    assert {(n, k) for n, c in chains.items() for k in c.outputs} == set(want)
    for B in (0, 1, 5):
        for (chain, kind), (frame, dtype) in want.items():
            assert output_spec(chains[chain], kind, B) == ((B,) + frame, dtype), (kind, B)
    for chain, kind in (("float", "iq"), ("float", None), ("q15", "mag_full"), ("q15", None),
                        ("window", "iq"), ("float", "bogus")):
        with pytest.raises(SpecanError) as e:
            output_spec(chains[chain], kind, 1)
        assert e.value.code == SA_EINVAL


def test_entry_point_table():
    import torch
    from fpga_real_time_fft_analyzer_amd.abi import SA_P12_FRAME_BYTES, SIGNATURES
    from fpga_real_time_fft_analyzer_amd.chain import _ARGS
    chains = _chains()
    f32, i16, p12 = torch.float32, torch.int16, torch.uint8
    want = {("float", f32): "sa_process_f32", ("float", i16): "sa_process_f32_i16",
            ("float", p12): "sa_process_f32_p12",
            ("q15", i16): {"iq": "sa_process_q15", "mag": "sa_process_q15_out", "marker": "sa_process_q15_out"},
            ("q15", p12): "sa_process_q15_p12",
            ("window", i16): "sa_filter_q15", ("window", p12): "sa_filter_q15_p12"}
    assert {(n, d) for n, c in chains.items() for d in c.inputs} == set(want)
    assert [list(c.inputs)[0] for c in chains.values()] == [f32, i16, i16]
    for (chain, dtype), name in want.items():
        chain = chains[chain]
        assert chain.inputs[dtype][0] == (SA_P12_FRAME_BYTES if dtype == p12 else N)
        for kind in chain.outputs:
            assert chain.inputs[dtype][1][kind][0] == (name[kind] if isinstance(name, dict) else name), (dtype, kind)
    # the argument list each entry point is called with is the one the binding declares for it
    for name, (takes_scale, takes_kind) in _ARGS.items():
        argtypes = SIGNATURES[name][1]
        assert (ctypes.c_float in argtypes) == takes_scale and argtypes.count(ctypes.c_int) == 1 + takes_kind, name
        assert len(argtypes) == 5 + takes_scale + takes_kind
    assert {call for c in chains.values() for _, calls in c.inputs.values() for call in calls.values()} == \
        {(name,) + form for name, form in _ARGS.items()}


# ---- N2 / N3 edges: framing front-end and UDP emitter (pure host logic)
def test_frame_cutter():
    from fpga_real_time_fft_analyzer_amd.ingest import FrameCutter
    fc = FrameCutter()
    x = np.arange(40000, dtype=np.int32) % 4096 - 2048
    out = fc.push(x[:10000])
    assert out.shape == (0, N) and fc.pending == 10000
    out = fc.push(x[10000:])
    assert out.shape == (2, N) and fc.pending == 40000 - 2 * N
    assert np.array_equal(out[0], x[:N]) and np.array_equal(out[1], x[N:2 * N])
    fo = FrameCutter(hop=N // 2)
    out = fo.push(x[:2 * N])
    assert out.shape == (3, N) and np.array_equal(out[1], x[N // 2:N // 2 + N]) and fo.pending == N // 2
    with pytest.raises(ValueError):
        FrameCutter(hop=0)
    with pytest.raises(ValueError):
        FrameCutter().push(np.array([40000]))


def test_udp_emit_loopback():
    import socket
    from fpga_real_time_fft_analyzer_amd.ingest import udp_emit
    g = load_golden("g6_frame.npz")
    frame = g["frame"].tobytes()
    rx = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    rx.setsockopt(socket.SOL_SOCKET, socket.SO_RCVBUF, 1 << 20)
    rx.bind(("127.0.0.1", 0))
    rx.settimeout(5.0)
    assert udp_emit(frame, rx.getsockname()) == 64
    asm = FrameCollector()
    got = None
    for _ in range(64):
        got = asm.add(rx.recv(2048), 0)
    rx.close()
    assert got == frame


def test_fft_regs_host(tmp_path):
    """The in-register FFT building blocks (csrc/fft_regs.hpp: radix-2 DIT of 4..32 points with compile-time
    twiddles, the packed complex product) compiled for the HOST from the same header the kernels include and
    checked against a naive float64 DFT (tests/cpp/test_fft_regs.cpp; <= 5e-7 max-norm relative)."""
    from native import standalone
    assert "fft32" in standalone(tmp_path, "test_fft_regs", sanitize=False)


def test_wide_step_split_accumulators_are_exact():
    """The wide Q2.14 step of the GPU kernel (cascade_q15.hip, filter_w14_kernel) never forms the 34-bit sum of
    or_iir_sos_q14: every tap -- and every NEGATED feedback tap, which reaches +32768 -- splits as c = 2^14 ch + cl with
    cl in [-8192, 8191], the two sums acc_l = 8192 + sum cl v and acc_h = sum ch v stay inside 32 bits at every partial sum,
    and (acc + 8192) >> 14 = acc_h + (acc_l >> 14) exactly.  Checked here on the host for random and extreme operands, so
    that the identity the kernel rests on is pinned without a GPU."""
    rng = np.random.default_rng(14)

    def split(c):
        cl = ((c + 8192) & 16383) - 8192
        return cl, (c - cl) >> 14
    taps = np.concatenate([rng.integers(-32768, 32768, (20000, 5)), np.array([[-32768] * 5, [32767] * 5, [-32768, 32767, -32768, 32767, -32768]])])
    vals = np.concatenate([rng.integers(-32768, 32768, (20000, 5)), np.array([[-32768] * 5, [-32768] * 5, [32767, -32768, 32767, -32768, 32767]])])
    eff = taps.astype(np.int64).copy()
    eff[:, 3:] = -eff[:, 3:]                                   # b0, b1, b2, -a1, -a2: the last two reach +32768
    cl, ch = split(eff)
    assert cl.min() >= -8192 and cl.max() <= 8191 and ch.min() >= -2 and ch.max() <= 2
    assert np.array_equal((ch << 14) + cl, eff)
    v = vals.astype(np.int64)
    part_l = 8192 + np.cumsum(cl * v, axis=1)
    part_h = np.cumsum(ch * v, axis=1)
    assert np.abs(part_l).max() < 2 ** 31 and np.abs(part_h).max() < 2 ** 31      # no partial sum wraps
    acc = (eff * v).sum(axis=1)
    assert np.array_equal((acc + 8192) >> 14, part_h[:, -1] + (part_l[:, -1] >> 14))


def test_fft_q15_paired_stage_addressing():
    """The index arithmetic of fft_q15_kernel (csrc/fft_q15.hip) restated in numpy on complex doubles: stage 0 from
    the input, the register passes (1,2), (3,4), (5,6) with their thread-to-butterfly maps, twiddle exponents, output
    positions and the two XOR swizzles.  With exact arithmetic the result must be the DFT in natural order, and every
    swizzled LDS access of a wave must touch 64 different banks."""
    rng = np.random.default_rng(5)
    n = 16384
    x = rng.standard_normal(n)
    W = np.exp(-2j * np.pi * np.arange(n) / n)

    def bf4(a, b, c, d, e):                                  # radix-4 DIF butterfly, outputs i' twiddled by W^(i' e)
        o = [a + b + c + d, a - 1j * b - c + 1j * d, a - b + c - d, a + 1j * b - c - 1j * d]
        return [o[i] * W[(i * e) % n] for i in range(4)]

    t = np.arange(1024)
    lane, wave = t & 63, t >> 6

    def banks_distinct(addr):                                # [1024] word addresses of one wave instruction per 64 lanes
        return all(len(set((addr[w * 64:(w + 1) * 64] & 63).tolist())) == 64 for w in range(16))

    buf = np.zeros(n, complex)
    for u in range(4):                                       # stage 0: bf = t + 1024 u, outputs at 4 bf + i'
        bf = t + 1024 * u
        o = bf4(x[bf], x[bf + 4096], x[bf + 8192], x[bf + 12288], bf)
        for i in range(4):
            buf[4 * bf + i] = o[i]
    # pass (1,2)
    v = [buf[t + 1024 * m] for m in range(16)]
    xx = [None] * 16
    for u in range(4):
        e1 = ((t + 1024 * u) >> 2) << 2
        o = bf4(v[u], v[u + 4], v[u + 8], v[u + 12], e1)
        for i in range(4):
            xx[4 * i + u] = o[i]
    j2 = (t >> 2) & 255
    ob = ((j2 << 6) | (t & 3)) ^ ((j2 & 15) << 2)
    buf2 = np.zeros(n, complex)
    plain = np.zeros(n, complex)                             # the same without the swizzle: Stockham order after three stages
    for ip in range(4):
        o = bf4(xx[4 * ip], xx[4 * ip + 1], xx[4 * ip + 2], xx[4 * ip + 3], j2 << 4)
        for i in range(4):
            addr = ob ^ ((4 * i + ip) << 2)
            assert banks_distinct(addr)
            buf2[addr] = o[i]
            plain[(j2 << 6) | (i << 4) | (ip << 2) | (t & 3)] = o[i]
    # pass (3,4)
    for m in range(16):
        addr = (t + 1024 * m) ^ (wave << 2)
        assert banks_distinct(addr)
        assert np.array_equal(buf2[addr], plain[t + 1024 * m])
    v = [buf2[(t + 1024 * m) ^ (wave << 2)] for m in range(16)]
    for u in range(4):
        o = bf4(v[u], v[u + 4], v[u + 8], v[u + 12], (wave + 16 * u) << 6)
        for i in range(4):
            xx[4 * i + u] = o[i]
    buf3 = np.zeros(n, complex)
    for ip in range(4):
        o = bf4(xx[4 * ip], xx[4 * ip + 1], xx[4 * ip + 2], xx[4 * ip + 3], wave << 8)
        for i in range(4):
            addr = (wave << 10) | ((4 * i + ip) << 6) | lane
            assert banks_distinct(addr)
            buf3[addr] = o[i]
    # pass (5,6)
    v = [buf3[t + 1024 * m] for m in range(16)]
    w = [None] * 16
    for u in range(4):
        o = bf4(v[u], v[u + 4], v[u + 8], v[u + 12], u * 1024)
        for i in range(4):
            w[4 * u + i] = o[i]
    out = np.zeros(n, complex)
    for u in range(4):
        o = bf4(w[u], w[u + 4], w[u + 8], w[u + 12], 0)
        for i in range(4):
            out[t + 1024 * (u + 4 * i)] = o[i]
    ref = np.fft.fft(x)
    assert np.abs(out - ref).max() <= 1e-9 * np.abs(ref).max()


def test_cascade_helper_wave_schedule():
    """The hand-over between a cascade wave and its helper wave (csrc/cascade_q15.hip: q15_helper_wave), interval by interval
    between workgroup barriers: within an interval the two waves never touch the same half of either ring, a flush only
    reads samples the cascade wrote in an EARLIER interval, and the flushes cover every sample of the frame exactly once."""
    tile, ring, nt, n = 256, 512, 64, 16384
    slot = lambda m: (m + 8) % ring                          # sample m lives in ring slot (m + 8) mod kRing
    written_in = {}                                          # sample -> interval in which the cascade stored it
    flushed = []
    for k in range(nt + 1):                                  # interval k: cascade tile k (k = nt: the drain)
        if k < nt:
            cas_samples = range(k * tile - 8, (k + 1) * tile - 8)
            cas_in_half = k & 1                              # input ring half the cascade reads
        else:
            # the drain.  The wide cascade runs one more iteration of its tile loop = four groups: the first stores the
            # frame's last eight samples, the other three store 24 "samples" beyond the frame into ring slots 8..31.
            # (The Q7 cascade runs the first group only: a subset.)
            cas_samples = range(nt * tile - 8, nt * tile + 24)
            assert {slot(m) for m in cas_samples} == set(range(32))
            cas_in_half = k & 1                              # and reads on in the input ring (a tile long consumed)
        cas_slots = {slot(m) for m in cas_samples}
        hlp_in_half = (k + 1) & 1 if k + 1 < nt else None    # input ring half the helper windows the next tile into
        if cas_in_half is not None and hlp_in_half is not None:
            assert cas_in_half != hlp_in_half
        if k >= 1:                                           # helper flushes samples [(k-1) tile - 8, k tile - 8)
            fl = range((k - 1) * tile - 8, k * tile - 8)
            fl_slots = {(((k - 1) * tile) + c) % ring for c in range(tile)}
            assert fl_slots == {slot(m) for m in fl}
            assert not (fl_slots & cas_slots)
            for m in fl:
                if m >= 0:
                    assert written_in[m] < k
                    flushed.append(m)
        for m in cas_samples:
            written_in[m] = k
    tail = range(nt * tile - 8, nt * tile)                   # after the last barrier: eight samples from slots 0..7
    assert {slot(m) for m in tail} == set(range(8)) and all(written_in[m] == nt for m in tail)
    flushed += list(tail)
    assert sorted(flushed) == list(range(n))
