"""CPU: the constant tables the kernels index (csrc/sa_tables.hpp), built and dumped on the host by
tests/cpp/test_sa_tables.cpp.  sa_create() needs a GPU, these functions do not: the window ROM, the Q15 twiddles and
their per-butterfly records, the float window, the three window layouts, the three float twiddle tables and the
cosine-window fit are checked here against the oracle, the golden ROM and numpy."""
import os

import numpy as np
import pytest

from conftest import N, load_golden
from native import standalone

TW_RECS = 4096 + 1024 + 256            # kSaTwRecs (csrc/sa_common.hpp)


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """{file name: array} of everything the program wrote, plus "stdout"."""
    d = tmp_path_factory.mktemp("sa_tables")
    stdout = standalone(d, "test_sa_tables", ["sa_tables.cpp"], sanitize=False, args=[str(d)])
    kinds = {"f64": np.float64, "f32": np.float32, "i16": np.int16, "u32": np.uint32}
    t = {fn: np.fromfile(str(d / fn), dtype=np.dtype(kinds[fn.rsplit(".", 1)[1]]).newbyteorder("<"))
         for fn in os.listdir(str(d)) if fn.rsplit(".", 1)[-1] in kinds}
    t["stdout"] = stdout
    return t


def test_window_rom(tables, oracle):
    rom = tables["rom.i16"]
    assert np.array_equal(rom, load_golden("g1_hann_rom.npz")["rom"])
    assert np.array_equal(rom, oracle.hann_rom_q15())


def test_q15_twiddles_and_records(tables, oracle):
    assert "q15_twiddles 1\n" in tables["stdout"]
    tq = tables["twq.u32"].reshape(N, 2)
    wr, wi = oracle.fxfft_twiddles()
    lo = lambda v: (v & 0xFFFF).astype(np.uint16).view(np.int16)
    hi = lambda v: (v >> 16).astype(np.uint16).view(np.int16)
    assert np.array_equal(lo(tq[:, 0]), wr) and np.array_equal(hi(tq[:, 0]), wi)
    assert np.array_equal(lo(tq[:, 1]), np.minimum(-wi.astype(np.int32), 32767).astype(np.int16))
    assert np.array_equal(hi(tq[:, 1]), wr)
    r = np.arange(TW_RECS)
    e = np.where(r < 4096, r, np.where(r < 5120, 4 * (r - 4096), 16 * (r - 5120)))
    want = np.concatenate([tq[e], tq[2 * e], tq[3 * e], np.zeros((TW_RECS, 2), np.uint32)], axis=1)
    assert np.array_equal(tables["twrec.u32"].reshape(TW_RECS, 8), want)


def test_float_window(tables, oracle):
    w = oracle.hann_f64().astype(np.float32)
    assert np.array_equal(tables["win.f64"].astype(np.float32), w)
    assert np.array_equal(tables["half.f32"], np.float32(0.5) * w)


def test_window_layouts_are_the_documented_permutations(tables):
    w = np.arange(N)                                   # the program lays out the ramp w[i] = i
    tr = tables["transpose.f32"]
    assert np.array_equal(tr.reshape(16, 256, 4), w.reshape(256, 16, 4).transpose(1, 0, 2))
    tr = tables["transpose.f64"]
    assert np.array_equal(tr.reshape(32, 256, 2), w.reshape(256, 32, 2).transpose(1, 0, 2))
    pa = tables["pass_a.f32"]
    assert np.array_equal(pa.reshape(16, 256, 2, 2), w.reshape(16, 2, 256, 2).transpose(0, 2, 1, 3))


def test_float_twiddles(tables):
    """twT, twB and twC against cos / sin in float64 at the angles documented in SaF32Tables (csrc/sa_common.hpp).
    Bound 2^-24: the entries are at most 1 in magnitude, so a float32 rounding of the exact value is within 2^-25, and
    one ulp of disagreement between two libm implementations in double cannot move it further than 2^-24."""
    def W(e, n):                                       # W_n^e as (cos, sin) of -2 pi e / n, e reduced first
        a = -2.0 * np.pi * (np.asarray(e) % n) / n
        return np.stack([np.cos(a), np.sin(a)], axis=-1)

    t = np.arange(256)
    want = np.empty((6, 256, 2, 2))
    for row, (k0, k1) in enumerate([(1, 2), (3, 4), (5, 6), (7, 8), (16, 24)]):
        want[row, :, 0] = W(k0 * t, 8192)
        want[row, :, 1] = W(k1 * t, 8192)
    want[5, :, 0] = W(4 * t, 16384)
    want[5, :, 1] = W(4 * ((t + 1) & 255), 16384)
    err_t = np.abs(tables["twT.f32"].reshape(6, 256, 2, 2) - want).max()
    p, b = np.meshgrid(np.arange(8), np.arange(16), indexing="ij")
    want = np.stack([W(2 * p * b, 256), W((2 * p + 1) * b, 256)], axis=2)
    err_b = np.abs(tables["twB.f32"].reshape(8, 16, 2, 2) - want).max()
    blk, e = np.meshgrid(np.arange(5), np.arange(5), indexing="ij")
    err_c = np.abs(tables["twC.f32"].reshape(5, 5, 2) - W(1024 * blk + e, 16384)).max()
    print(f"twT {err_t:.3e} twB {err_b:.3e} twC {err_c:.3e}")
    assert max(err_t, err_b, err_c) <= 2.0 ** -24


def test_fit_cosine_window(tables):
    """Hann and Hamming are accepted with both coefficients within 1.5e-7 (the function's own residual bound at peak 1);
    Blackman, the all-zero table and a table holding one NaN are refused."""
    fits = {}
    for line in tables["stdout"].splitlines():
        f = line.split()
        if f and f[0] == "fit":
            fits[f[1]] = (int(f[2]), float(f[3]), float(f[4]))
    print(fits)
    assert sorted(fits) == ["blackman", "hamming", "hann", "nan", "zero"]
    for name, a0, a1 in (("hann", 0.5, 0.5), ("hamming", 0.54, 0.46)):
        ok, f0, f1 = fits[name]
        assert ok == 1 and abs(f0 - a0) <= 1.5e-7 and abs(f1 - a1) <= 1.5e-7, (name, fits[name])
    for name in ("blackman", "zero", "nan"):
        assert fits[name][0] == 0, (name, fits[name])
