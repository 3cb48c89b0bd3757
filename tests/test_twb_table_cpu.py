"""CPU: the pass-B twiddle table as the host builds and uploads it (csrc/sa_tables.cpp, float_twiddles -> SaF32Tables::twB).

The fused float kernels copy this table into LDS once per workgroup -- threads 0..127 move one 16-byte quad each -- and pass B
reads quad [p][b] for its lane's b = lane & 15.  What is checked here is the layout that copy and those reads rely on:
128 quads (2 KiB), quad [p][b] = (W_256^(2p b), W_256^((2p+1) b)), which read as rows k = 2p + h is the plain 16 x 16 table
W_256^(k b).  Bound 2^-24 as in tests/test_host_tables.py: the entries are at most 1 in magnitude, a float32 rounding of the
exact value is within 2^-25, and two libm implementations differ by at most an ulp of the double."""
import numpy as np
import pytest

from native import standalone


@pytest.fixture(scope="module")
def twb(tmp_path_factory):
    d = tmp_path_factory.mktemp("twb_table")
    standalone(d, "test_sa_tables", ["sa_tables.cpp"], sanitize=False, args=[str(d)])
    return np.fromfile(str(d / "twB.f32"), dtype="<f4")


def test_twb_is_the_16_by_16_table_of_w256(twb):
    assert twb.size == 8 * 16 * 4                      # 128 quads: one per copying thread, 2 KiB of LDS
    rows = twb.reshape(8, 16, 2, 2).transpose(0, 2, 1, 3).reshape(16, 16, 2)      # [k = 2p + h][b][re, im]
    k, b = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    ang = -2.0 * np.pi * ((k * b) % 256) / 256.0
    want = np.stack([np.cos(ang), np.sin(ang)], axis=-1)
    err = np.abs(rows - want).max()
    print(f"FIGURE twB: worst |entry - W_256^(k b)| {err:.3e}")
    assert err <= 2.0 ** -24
    # the identity entries are exact: pass B skips the product for k = 0 and relies on (1, 0) for b = 0
    assert np.array_equal(rows[0], np.tile(np.float32([1, 0]), (16, 1)))
    assert np.array_equal(rows[:, 0], np.tile(np.float32([1, 0]), (16, 1)))
    # symmetric in k and b, as W^(k b) is: a transposed upload would not show, a shifted or strided one does
    assert np.array_equal(rows, rows.transpose(1, 0, 2))
