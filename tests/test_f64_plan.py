"""CPU: the float64-state IIR plan (sa_iir_plan_from_sos_f64) and a numpy emulation of iir_f64.hip's algebra.

The kernel evaluates every section as 256 threads x 2 chunks of 32 samples: chunk end states from zero state
(predictor taps, block Horner over two half chunks), an affine scan over the 512 chunks (in-row Kogge-Stone over 16
lanes, then over the 16 row totals), then the DF2T recursion of scipy.signal.sosfilt from the true start states -- all
in float64, with the plan read from the library.  The emulation below follows that structure step by step.
"""
import numpy as np
import pytest

from conftest import N, load_golden, rel_maxnorm

SEC_DOUBLES = 6 + 32 + 4 + 4 + 16 + 16 + 64

# every case named in profiles/r4_fuzz.txt (the float32 path's outliers), seed -> case indices
R4_NAMED = {
    7: [600, 1389, 752, 1195, 546, 40, 1435, 1101, 1203, 1233, 9, 892],
    11: [929, 765, 269, 1256, 108, 1040, 859, 752, 819, 1301, 962, 1075],
    23: [134, 1188, 549, 701, 56, 142, 99, 289, 1095, 160, 1244, 1128],
}

# the RTL's default taps as reals (imp/filter_pkg.vhd:54-68): ALPHA and BETA alternate over six stages
_ALPHA = [14 / 128, 0, -14 / 128, 1, 21 / 128, 107 / 128]
_BETA = [15 / 128, 0, -15 / 128, 1, -21 / 128, 107 / 128]
RTL_DEFAULT = np.array([_ALPHA, _BETA] * 3)


def parse_plan_f64(plan):
    """SaIirF64 as written by sa_iir_plan_from_sos_f64: hdr[4], then 6 x {c[6], m[16][2], p16, pc, plev[4], prow[4],
    lane[16]}, every matrix row-major [[m0, m1], [m2, m3]]."""
    assert plan.size == 4 + 6 * SEC_DOUBLES
    nsec = int(plan[0])
    secs = []
    off = 4
    for _ in range(6):
        c = plan[off:off + 6]; off += 6
        m = plan[off:off + 32].reshape(16, 2); off += 32
        p16 = plan[off:off + 4].reshape(2, 2); off += 4
        pc = plan[off:off + 4].reshape(2, 2); off += 4
        plev = plan[off:off + 16].reshape(4, 2, 2); off += 16
        prow = plan[off:off + 16].reshape(4, 2, 2); off += 16
        lane = plan[off:off + 64].reshape(16, 2, 2); off += 64
        secs.append(dict(c=c, m=m, p16=p16, pc=pc, plev=plev, prow=prow, lane=lane))
    return nsec, secs


def _ks(z, mats):
    """Inclusive Kogge-Stone affine scan along axis -2 (16 entries, zero fill): z += P_lev * shifted(z)."""
    for lev, d in enumerate((1, 2, 4, 8)):
        u = np.zeros_like(z)
        u[..., d:, :] = z[..., :-d, :]
        z = z + u @ mats[lev].T
    return z


def emulate_f64(plan, xw):
    """The float64 algebra of iir_f64.hip on one windowed frame xw (float64 [N]); returns y in float64."""
    nsec, secs = parse_plan_f64(plan)
    v = np.asarray(xw, np.float64).reshape(256, 2, 32).copy()       # [thread][chunk][j]
    for s in range(nsec):
        k = secs[s]
        m = k["m"]
        # predict: z = A^16 (sum_{j<16} m[j] v[j]) + sum_{j<16} m[j] v[16 + j]
        first = np.einsum("tcj,js->tcs", v[:, :, :16], m)
        second = np.einsum("tcj,js->tcs", v[:, :, 16:], m)
        z = first @ k["p16"].T + second                              # [thread][chunk][state]
        zA, zB = z[:, 0, :], z[:, 1, :]
        T = zA @ k["pc"].T + zB
        inc = _ks(T.reshape(16, 16, 2), k["plev"])                   # [row][lane][state]
        exc = np.zeros_like(inc)
        exc[:, 1:, :] = inc[:, :-1, :]
        rows = _ks(inc[:, 15, :].reshape(1, 16, 2), k["prow"])[0]
        C = np.zeros((16, 2))
        C[1:] = rows[:-1]
        sA = (exc + np.einsum("iab,rb->ria", k["lane"], C)).reshape(256, 2)
        sB = sA @ k["pc"].T + zA
        s1 = np.stack([sA[:, 0], sB[:, 0]], axis=1)
        s2 = np.stack([sA[:, 1], sB[:, 1]], axis=1)
        b0, b1, b2, a1, a2 = k["c"][:5]
        for j in range(32):
            x = v[:, :, j]
            y = b0 * x + s1
            s1 = b1 * x + s2 - a1 * y
            s2 = b2 * x - a2 * y
            v[:, :, j] = y
    return v.reshape(-1)


def _named_cases():
    import fuzz_parity
    out = []
    for seed, idx in R4_NAMED.items():
        want = set(idx)
        for case, sos, label, x in fuzz_parity.cases(seed, max(idx) + 1):
            if case in want:
                out.append((f"seed {seed} case {case} {label}", sos, x))
    return out


def _fixed_cases():
    g = load_golden("g3_fp32_frames.npz")
    sos = g["sos"]
    n = np.arange(N)
    rng = np.random.default_rng(5)
    tone = (0.7 * np.sin(2 * np.pi * 0.031 * n) + 0.05 * rng.standard_normal(N)).astype(np.float32)[None, :]
    return [("headline Butterworth", sos, g["x"][:2]), ("RTL default taps", RTL_DEFAULT, tone),
            ("padded 3-section cascade", sos[:3], g["x"][:1])]


def _check(oracle, name, sos, x):
    from scipy.signal import sosfilt
    from fpga_real_time_fft_analyzer_amd.chain import iir_plan_f64_from_sos
    plan = iir_plan_f64_from_sos(sos)
    hann = oracle.hann_f64()
    _, _, mag = oracle.chain_fp(x, sos)
    for i in range(x.shape[0]):
        xw = x[i].astype(np.float64) * hann
        ref = sosfilt(sos, xw)
        y = emulate_f64(plan, xw)
        assert rel_maxnorm(y[None, :], ref[None, :]) <= 1e-9, name
        spec = np.abs(np.fft.rfft(y.astype(np.float32).astype(np.float64)))   # y rounded once, as the kernel stores it
        assert rel_maxnorm(spec[None, :], mag[i:i + 1, :N // 2 + 1]) <= 2e-6, name


def test_f64_plan_algebra_fixed_cascades(hip_lib_built, oracle):
    for name, sos, x in _fixed_cases():
        _check(oracle, name, sos, x)


def test_f64_plan_algebra_on_the_float32_outliers(hip_lib_built, oracle):
    """Every design named in profiles/r4_fuzz.txt -- up to 65x above 1e-5 on the float32 path -- drawn without a GPU."""
    cases = _named_cases()
    assert len(cases) == sum(len(v) for v in R4_NAMED.values())
    for name, sos, x in cases:
        _check(oracle, name, sos, x)


def test_f64_plan_layout_and_padding(hip_lib_built):
    from fpga_real_time_fft_analyzer_amd.chain import iir_plan_f64_from_sos
    sos = np.array([[0.2, 0.1, 0.05, 2.0, -0.6, 0.3]])
    nsec, secs = parse_plan_f64(iir_plan_f64_from_sos(sos))
    assert nsec == 2
    b0, b1, b2, a0, a1, a2 = sos[0] / sos[0, 3]                   # a0-normalised
    assert np.array_equal(secs[0]["c"], [b0, b1, b2, a1, a2, 0.0])
    A = np.array([[-a1, 1.0], [-a2, 0.0]])
    Bv = np.array([b1 - a1 * b0, b2 - a2 * b0])
    assert np.allclose(secs[0]["m"][15], Bv, rtol=0, atol=1e-15)
    assert np.allclose(secs[0]["m"][0], np.linalg.matrix_power(A, 15) @ Bv, rtol=1e-12, atol=1e-18)
    assert np.allclose(secs[0]["pc"], np.linalg.matrix_power(A, 32), rtol=1e-12, atol=1e-18)
    assert np.allclose(secs[0]["plev"][3], np.linalg.matrix_power(A, 512), rtol=1e-12, atol=1e-30)
    assert np.allclose(secs[0]["lane"][5], np.linalg.matrix_power(A, 320), rtol=1e-12, atol=1e-30)
    # the padding section is the identity: y = 1 * x, every tap and every transition power of 2 and more is zero
    pad = secs[1]
    assert np.array_equal(pad["c"], [1, 0, 0, 0, 0, 0]) and not pad["m"].any() and not pad["pc"].any()
    assert np.array_equal(pad["lane"][0], np.eye(2)) and not pad["lane"][1:].any()
    assert all(int(parse_plan_f64(iir_plan_f64_from_sos(np.tile(sos, (n, 1))))[0]) == p
               for n, p in ((1, 2), (2, 2), (3, 4), (4, 4), (5, 6), (6, 6)))


def test_f64_plan_rejects_bad_sos(hip_lib_built):
    """The same bad inputs as sa_iir_plan_from_sos (test_host_logic.py::test_iir_plan_rejects_bad_sos)."""
    from fpga_real_time_fft_analyzer_amd.abi import SpecanError
    from fpga_real_time_fft_analyzer_amd.chain import iir_plan_f64_from_sos
    with pytest.raises(SpecanError):
        iir_plan_f64_from_sos(np.zeros((7, 6)))
    with pytest.raises(SpecanError):
        iir_plan_f64_from_sos(np.array([[1, 0, 0, 0, 0, 0.0]]))     # a0 = 0
    with pytest.raises(SpecanError):
        iir_plan_f64_from_sos(np.array([[1, 0, 0, np.inf, 0, 0.0]]))
    assert int(iir_plan_f64_from_sos(np.zeros((0, 6)))[0]) == 0
