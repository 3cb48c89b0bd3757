"""GPU: the level histogram (include/specan_hist.h: sa_hist_f32 of libspecan_hist.so), through SpectrumChain.level_hist,
SpectrumChain.persistence_f32 and the C entry point.

Every comparison is exact, torch.equal on the uint32 counters, against the numpy mirror frames.hist_of_rows, whose probes
tests/test_f32_hist_cpu.py works out by hand; the probes are part of the data here, and their expected counts are asserted
again on the device's.

The kernel's ownership (csrc/hist_f32.hip): a workgroup has one group of A rows and one tile of 256 bins; wave w of
n = min(max(A, 4), 16) takes the rows w, w + n, ..., eight of them at a time while it has eight left (A >= 8 n) and one at a
time after; a lane holds four adjacent bins.  The shapes below have A below, at and above the number of waves, A that leaves
a wave with seven, eight and nine rows, ranges that cut a lane's quad (W = 1, 2), a tile, or lie inside one, every bucket
and L on both sides of every power of two.  Where G x tiles < 256 and A >= 64 the rows of a group are cut into
min(ceil(512 / (G tiles)), A / 32) slices that merge into a zeroed output: the shapes stand on both sides of each of the two
conditions (G x tiles 192 and 256; A 63, 64 and 65) and have slices of unequal length (131 rows in 4)."""
import ctypes

import numpy as np
import pytest

from conftest import N, load_golden
from gpu_support import ch, lds_fill, to_device, torch_mod  # noqa: F401 (fixtures)
from test_gpu_f32_peaks import _inputs, _tones

pytestmark = pytest.mark.gpu

SA_OK, SA_EINVAL, SA_ESHAPE = 0, -1, -2
# rows, A, W, L, lo, hi: the table of the issue, then A around the waves' row counts and ranges inside and across tiles
SHAPES = [(1, 1, 1, 2, 0, N), (3, 3, 1, 64, 0, N), (5, 5, 2, 3, 2, 16382), (34, 17, 4, 64, 4, 260), (12, 4, 16, 33, 16368, N),
          (7, 1, 64, 64, 0, N), (66, 33, 8, 5, 248, 16136), (64, 64, 32, 17, 0, N),
          (3, 3, 1, 9, 1, 16383), (4, 2, 2, 4, 254, 258), (2, 2, 1, 32, 300, 301), (6, 6, 4, 8, 260, 508), (16, 16, 8, 16, 248, 264),
          (8, 4, 64, 2, 0, 64), (5, 5, 64, 7, 16320, N), (10, 5, 1, 65 - 1, 255, 257), (9, 9, 16, 63, 4096, 8192),
          (262, 131, 4, 7, 0, 1024), (127, 127, 2, 6, 510, 770), (145, 145, 32, 12, 16000, N),
          (524, 131, 8, 9, 0, N), (192, 64, 16, 20, 0, N), (63, 63, 4, 5, 0, 512), (130, 65, 1, 3, 255, 513)]


def _edges(L, seed=0):
    """L - 1 float32 edges across exp(+-18), a few of them equal"""
    e = np.exp(np.linspace(-18.0, 18.0, L - 1)).astype(np.float32)
    if L > 8:
        e[5] = e[4]                                               # an empty level
    return e


def _data(rows, edges, seed):
    """float32 [rows, N]: exp(uniform +-20) with signs mixed and a fifth of the points exactly on an edge or one ulp off"""
    rng = np.random.default_rng(seed)
    pts = np.exp(rng.uniform(-20.0, 20.0, size=(rows, N))).astype(np.float32)
    tie = rng.random((rows, N)) < 0.2
    on = rng.choice(edges, size=(rows, N)).view(np.int32) + rng.integers(-1, 2, size=(rows, N), dtype=np.int32)
    pts[tie] = np.maximum(on, 0).view(np.float32)[tie]
    pts[rng.random((rows, N)) < 0.1] *= -1.0
    return pts


def _want(torch, pts, edges, **kw):
    from fpga_real_time_fft_analyzer_amd import frames
    return torch.from_numpy(frames.hist_of_rows(pts, edges, **kw)).to(torch.int64)


def _host(t):
    """uint32 counters on the host, widened: torch compares and sums int64, not uint32"""
    import torch
    assert t.dtype == torch.uint32
    return t.cpu().to(torch.int64)


def _hist(ch, torch, x, edges, **kw):
    """level_hist on the device tensor -> the counters [G, C, L] on the host, as int64"""
    got = ch.level_hist(x, edges, **kw)
    assert got.dtype == torch.uint32 and got.is_contiguous() and got.is_cuda
    return _host(got)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_shapes_equal_the_mirror(ch, torch_mod, shape):
    rows, A, W, L, lo, hi = shape
    edges = _edges(L)
    pts = _data(rows, edges, 1900 + rows + L)
    got = _hist(ch, torch_mod, to_device(torch_mod, pts), edges, group=A, bucket=W, lo=lo, hi=hi)
    want = _want(torch_mod, pts, edges, group=A, bucket=W, lo=lo, hi=hi)
    assert tuple(got.shape) == (rows // A, (hi - lo) // W, L) and torch_mod.equal(got, want), shape
    assert (got.sum(dim=2) == A * W).all().item()


def test_hand_probes_on_the_device(ch, torch_mod):
    """The probes of tests/test_f32_hist_cpu.py with their expected counts written out."""
    torch = torch_mod
    # on an edge, one ulp below it and one above: 1.0 at bin 3, 0x3F7FFFFF at bin 700, 0x3F800001 at bin 16383, zeros elsewhere
    pts = np.zeros((1, N), np.float32)
    pts.view(np.uint32)[0, [3, 700, 16383]] = (0x3F800000, 0x3F7FFFFF, 0x3F800001)
    got = _hist(ch, torch, to_device(torch, pts), [1.0])
    assert tuple(got.shape) == (1, N, 2)
    assert got[0, 3].tolist() == [0, 1] and got[0, 700].tolist() == [1, 0] and got[0, 16383].tolist() == [0, 1]
    assert int(got[0, :, 1].sum()) == 2 and int(got[0, :, 0].sum()) == N - 2
    # the specials: edges (+0.0, 2.5, 1e30): NaN, +inf -> 3; -3.0 as 3.0 -> 2; 2.0 -> 1; the denormal of bits 1 -> 1 (above
    # the edge +0.0); -0.0 and the zeros -> 1 (equal to the edge +0.0): level 0 is empty
    pts = np.zeros((1, N), np.float32)
    for b, v in ((11, np.nan), (222, np.inf), (3333, -3.0), (4444, 2.0), (5555, 1e-45), (6666, -0.0)):
        pts[0, b] = v
    got = _hist(ch, torch, to_device(torch, pts), [0.0, 2.5, 1e30])
    for b, level in ((11, 3), (222, 3), (3333, 2), (4444, 1), (5555, 1), (6666, 1), (0, 1)):
        assert got[0, b].tolist() == [int(l == level) for l in range(4)], b
    assert got[0].sum(dim=0).tolist() == [0, N - 3, 1, 2]
    got = _hist(ch, torch, to_device(torch, pts), [1e-45, np.inf], bucket=64)          # the denormal on its edge; +inf on its
    assert got[0].sum(dim=0).tolist() == [N - 5, 3, 2] and got[0, 5555 // 64].tolist() == [63, 1, 0]
    assert got[0, 222 // 64].tolist() == [63, 0, 1] and got[0, 11 // 64].tolist() == [63, 0, 1]
    # L = 64, 63 distinct edges 1..63, the value l + 0.5 planted at bin 100 l + 7 of a row of 0.25 -> one count in level l
    pts = np.full((1, N), 0.25, np.float32)
    pts[0, 100 * np.arange(64) + 7] = np.arange(64) + 0.5
    got = _hist(ch, torch, to_device(torch, pts), np.arange(1, 64, dtype=np.float32))
    for l in range(64):
        assert got[0, 100 * l + 7].tolist() == [int(k == l) for k in range(64)], l
    assert got[0].sum(dim=0).tolist() == [N - 63] + [1] * 63
    # equal edges give empty levels: (1, 1, 1, 2)
    pts = np.zeros((2, N), np.float32)
    pts[0, :] = 1.0
    pts[1, :] = 1.5
    pts[1, 9] = 0.5
    got = _hist(ch, torch, to_device(torch, pts), [1.0, 1.0, 1.0, 2.0], group=2, bucket=2)
    assert got[0, 0].tolist() == [0, 0, 0, 4, 0] and got[0, 4].tolist() == [1, 0, 0, 3, 0]
    assert got[0].sum(dim=0).tolist() == [1, 0, 0, 2 * N - 1, 0]
    # bins outside [lo, hi) do not exist
    pts = np.ones((1, N), np.float32)
    pts[0, 999] = pts[0, 3000] = np.nan
    got = _hist(ch, torch, to_device(torch, pts), [2.0], lo=1000, hi=3000, bucket=8)
    assert tuple(got.shape) == (1, 250, 2) and got[0].sum(dim=0).tolist() == [2000, 0]


def test_a_counter_beyond_16_bits(ch, torch_mod):
    """A = 1025 rows of the constant 2.0 at W = 64: 1025 * 64 = 65 600 points per column, all in the level above the edges."""
    torch = torch_mod
    x = torch.full((1025, N), 2.0, dtype=torch.float32, device="cuda")
    got = _hist(ch, torch, x, [1.0, 1.5], bucket=64)
    assert tuple(got.shape) == (1, 256, 3)
    assert (got[0, :, 2] == 65600).all().item() and not got[0, :, :2].any().item()


def test_massive_same_cell_contention(ch, torch_mod):
    torch = torch_mod
    edges = np.arange(1, 64, dtype=np.float32)
    x = torch.full((64, N), 40.5, dtype=torch.float32, device="cuda")
    got = _hist(ch, torch, x, edges, bucket=16)                   # one cell per column takes every add
    assert (got[0, :, 40] == 64 * 16).all().item() and int(got.sum()) == 64 * N
    # 1.0 and the float below it, alternating by bin and by row, around the edge 1.0
    pts = np.empty((32, N), np.uint32)
    pts[:] = 0x3F800000
    pts[0::2, 0::2] = pts[1::2, 1::2] = 0x3F7FFFFF
    pts = pts.view(np.float32)
    for W in (1, 16, 64):
        got = _hist(ch, torch, to_device(torch, pts), [0.5, 1.0, 2.0], group=32, bucket=W)
        assert (got[0, :, 1] == 16 * W).all().item() and (got[0, :, 2] == 16 * W).all().item()
        assert torch.equal(got, _want(torch, pts, [0.5, 1.0, 2.0], group=32, bucket=W))


def test_nan_rows_stay_inside_their_own_group(ch, torch_mod):
    torch = torch_mod
    edges = _edges(16)
    data = _data(3, edges, 1950)
    nan_row, inf_row = np.full((1, N), np.nan, np.float32), np.full((1, N), np.inf, np.float32)
    pts = np.concatenate([nan_row, data[:1], nan_row, data[1:2], inf_row, data[2:], nan_row, nan_row])
    x = to_device(torch, pts)
    got = _hist(ch, torch, x, edges, group=1, bucket=4)
    assert torch.equal(got, _want(torch, pts, edges, group=1, bucket=4))
    for r in (0, 2, 4, 6, 7):
        assert (got[r, :, 15] == 4).all().item() and not got[r, :, :15].any().item()
    for r in (1, 3, 5):
        assert torch.equal(got[r:r + 1], _hist(ch, torch, x[r:r + 1], edges, group=1, bucket=4))
    got = _hist(ch, torch, x, edges, group=2, bucket=4)
    assert torch.equal(got, _want(torch, pts, edges, group=2, bucket=4))
    assert (got[3, :, 15] == 8).all().item() and (got[:3, :, 15] >= 4).all().item()


def _c_edges(values):
    return (ctypes.c_float * len(values))(*values)


def test_exactly_the_output_bytes_are_written_and_a_refused_call_writes_nothing(ch, torch_mod):
    from fpga_real_time_fft_analyzer_amd import abi
    from fpga_real_time_fft_analyzer_amd.abi import SpecanError
    torch = torch_mod
    L = abi.hist_lib()
    stream = torch.cuda.current_stream().cuda_stream
    guard = 4096
    for rows, A, log2w, nlev, lo, hi in ((6, 3, 0, 5, 1, 16383), (6, 2, 4, 64, 0, N), (4, 4, 6, 2, 64, 128), (5, 1, 2, 33, 252, 16380),
                                         (134, 67, 3, 9, 8, 16376)):
        edges = _edges(nlev)
        pts = _data(rows, edges, 1960 + nlev)
        x = to_device(torch, pts)
        G, cols = rows // A, (hi - lo) >> log2w
        n = G * cols * nlev * 4
        buf = torch.full((guard + n + guard,), 0xA5, dtype=torch.uint8, device="cuda")        # no zeroed buffer
        assert L.sa_hist_f32(x.data_ptr(), buf.data_ptr() + guard, rows, A, log2w, nlev, _c_edges(edges), lo, hi, stream) == SA_OK
        assert L.sa_hist_last_error() == b""
        torch.cuda.synchronize()
        assert (buf[:guard] == 0xA5).all().item() and (buf[guard + n:] == 0xA5).all().item()
        got = _host(buf[guard:guard + n].view(torch.uint32).view(G, cols, nlev))
        assert torch.equal(got, _want(torch, pts, edges, group=A, bucket=1 << log2w, lo=lo, hi=hi)), (rows, A, log2w, nlev)
    # refused calls: the code of sa_hist_check for the same arguments, its text, and nothing written
    rows, nlev, edges = 4, 4, [1.0, 2.0, 3.0]
    out = torch.full((rows * N * nlev * 4 + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    flat = torch.zeros((rows * N + 64,), dtype=torch.float32, device="cuda")
    before = flat.clone()
    p_in, p_out = flat.data_ptr(), out.data_ptr()
    nan, n_in = float("nan"), rows * N * 4
    for tag, args, code, words in (
            ("in 4 bytes off", (p_in + 4, p_out, rows, 2, 0, nlev, edges, 0, N), SA_EINVAL, "`in` must be 16-byte aligned"),
            ("out 2 bytes off", (p_in, p_out + 2, rows, 2, 0, nlev, edges, 0, N), SA_EINVAL, "`out` must be 4-byte aligned"),
            ("out inside in", (p_in, p_in + n_in - 4, rows, 2, 0, nlev, edges, 0, N), SA_EINVAL, "overlap"),
            ("in inside out", (p_out + 64, p_out, rows, 1, 0, nlev, edges, 0, N), SA_EINVAL, "overlap"),
            ("NULL", (p_in, 0, rows, 2, 0, nlev, edges, 0, N), SA_EINVAL, "NULL"),
            ("group 0", (p_in, p_out, rows, 0, 0, nlev, edges, 0, N), SA_EINVAL, "group must"),
            ("group 3", (p_in, p_out, rows, 3, 0, nlev, edges, 0, N), SA_ESHAPE, "multiple of group"),
            ("log2w 7", (p_in, p_out, rows, 2, 7, nlev, edges, 0, N), SA_EINVAL, "log2w"),
            ("nlev 65", (p_in, p_out, rows, 2, 0, 65, edges, 0, N), SA_EINVAL, "nlev"),
            ("nlev 1", (p_in, p_out, rows, 2, 0, 1, edges, 0, N), SA_EINVAL, "nlev"),
            ("lo = hi", (p_in, p_out, rows, 2, 0, nlev, edges, 9, 9), SA_EINVAL, "range"),
            ("lo off the bucket", (p_in, p_out, rows, 2, 3, nlev, edges, 4, N), SA_EINVAL, "range"),
            ("a NaN edge", (p_in, p_out, rows, 2, 0, nlev, [1.0, nan, 3.0], 0, N), SA_EINVAL, "edges[1]"),
            ("a negative edge", (p_in, p_out, rows, 2, 0, nlev, [-0.0, 2.0, 3.0], 0, N), SA_EINVAL, "edges[0]"),
            ("edges that decrease", (p_in, p_out, rows, 2, 0, nlev, [1.0, 3.0, 2.0], 0, N), SA_EINVAL, "edges[2] is below"),
            ("negative rows", (p_in, p_out, -1, 2, 0, nlev, edges, 0, N), SA_ESHAPE, "negative")):
        a_in, a_out, r, A, log2w, nl, ed, lo, hi = args
        assert L.sa_hist_check(a_in, a_out, r, A, log2w, nl, _c_edges(ed), lo, hi) == code, tag
        assert L.sa_hist_f32(a_in, a_out, r, A, log2w, nl, _c_edges(ed), lo, hi, stream) == code, tag
        assert words in L.sa_hist_last_error().decode(), (tag, L.sa_hist_last_error())
    assert L.sa_hist_f32(p_in, p_out, rows, 2, 0, nlev, None, 0, N, stream) == SA_EINVAL and b"NULL edges" in L.sa_hist_last_error()
    torch.cuda.synchronize()
    assert (out == 0xA5).all().item() and torch.equal(flat, before)
    assert L.sa_hist_f32(0, 0, 0, 2, 0, nlev, _c_edges(edges), 0, N, stream) == SA_OK and L.sa_hist_last_error() == b""
    # `out` right behind `in`: touching is fine
    edges = _edges(5)
    pts = _data(2, edges, 1970)
    n_in, n_out = 2 * N * 4, 1 * (N // 4) * 5 * 4
    packed = torch.zeros((n_in + n_out,), dtype=torch.uint8, device="cuda")
    packed[:n_in] = to_device(torch, pts).view(torch.uint8).view(-1)
    base = packed.data_ptr()
    assert L.sa_hist_f32(base, base + n_in, 2, 2, 2, 5, _c_edges(edges), 0, N, stream) == SA_OK
    torch.cuda.synchronize()
    got = _host(packed[n_in:].view(torch.uint32).view(1, N // 4, 5))
    assert torch.equal(got, _want(torch, pts, edges, group=2, bucket=4))
    # through the wrapper: shapes and dtypes before any device call
    x = to_device(torch, pts)
    for code, args, kw in ((SA_ESHAPE, (x[:, :N // 2], edges), {}), (SA_EINVAL, (x.double(), edges), {}), (SA_EINVAL, (x.cpu(), edges), {}),
                           (SA_ESHAPE, (torch.stack([x, x], dim=2).contiguous(), edges), {}),
                           (SA_ESHAPE, (x, edges), dict(group=3)), (SA_EINVAL, (x, edges), dict(group=0)),
                           (SA_ESHAPE, (x, edges), dict(out=torch.empty((1, N, 4), dtype=torch.uint32, device="cuda"))),
                           (SA_ESHAPE, (x, edges), dict(out=torch.empty((1, N, 5), dtype=torch.int32, device="cuda"))),
                           (SA_ESHAPE, (x, edges), dict(group=1, out=torch.empty((1, N, 5), dtype=torch.uint32, device="cuda"))),
                           (SA_ESHAPE, (x, edges), dict(out=torch.empty((1, N, 5), dtype=torch.uint32)))):
        with pytest.raises(SpecanError) as e:
            ch.level_hist(*args, **kw)
        assert e.value.code == code, (args[0].shape, kw)
    assert ch.level_hist(torch.empty((0, N), dtype=torch.float32, device="cuda"), edges, bucket=64).shape == (0, 256, 5)
    mine = torch.empty((2, N // 16, 5), dtype=torch.uint32, device="cuda")
    got = ch.level_hist(x, edges, group=1, bucket=16, out=mine)
    assert got.data_ptr() == mine.data_ptr() and torch.equal(_host(mine), _want(torch, pts, edges, group=1, bucket=16))


def test_poisoned_lds(ch, torch_mod, lds_fill):
    """lds_fill(P) with P = 0xFFFFFFFF and 0x7F800000, then the call on the same stream: the counts of the mirror.  A launch
    that did not zero its counters, or read an edge it did not plant, shows here."""
    torch = torch_mod
    for rows, A, W, nlev, lo, hi in ((4, 2, 1, 64, 0, N), (6, 6, 16, 33, 0, N), (3, 1, 4, 3, 252, 1028), (20, 20, 64, 64, 0, N),
                                     (96, 96, 1, 64, 0, N)):
        edges = _edges(nlev)
        pts = _data(rows, edges, 1980 + nlev)
        x = to_device(torch, pts)
        want = _want(torch, pts, edges, group=A, bucket=W, lo=lo, hi=hi)
        for word in (0xFFFFFFFF, 0x7F800000):
            lds_fill(word)
            assert torch.equal(_hist(ch, torch, x, edges, group=A, bucket=W, lo=lo, hi=hi), want), (hex(word), rows, A, W, nlev)


def test_two_calls_back_to_back(ch, torch_mod):
    torch = torch_mod
    e1, e2 = _edges(64), _edges(7) * np.float32(3.0)
    pts = _data(8, e1, 1990)
    x = to_device(torch, pts)
    o1 = torch.empty((2, N // 16, 64), dtype=torch.uint32, device="cuda")
    o2 = torch.empty((2, N // 16, 7), dtype=torch.uint32, device="cuda")
    ch.level_hist(x, e1, group=4, bucket=16, out=o1)
    ch.level_hist(x, e2, group=4, bucket=16, out=o2)
    torch.cuda.synchronize()
    assert torch.equal(_host(o1), _want(torch, pts, e1, group=4, bucket=16))
    assert torch.equal(_host(o2), _want(torch, pts, e2, group=4, bucket=16))


def test_capture_and_replay_keeps_the_captured_edges(ch, torch_mod):
    """The call captures without a warm-up -- it is one launch with its edges in the launch's arguments -- and a replay after
    the host array of edges has been overwritten still counts against the captured ones, on the input as it is then."""
    from fpga_real_time_fft_analyzer_amd import abi
    torch = torch_mod
    L = abi.hist_lib()
    edges = _edges(17)
    held = _c_edges(edges)
    first, second = _data(6, edges, 1991), _data(6, edges, 1992)
    x = to_device(torch, first)
    out = torch.empty((2, N // 8, 17), dtype=torch.uint32, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = L.sa_hist_f32(x.data_ptr(), out.data_ptr(), 6, 3, 3, 17, held, 0, N, torch.cuda.current_stream().cuda_stream)
    assert rc == SA_OK
    for j in range(16):
        held[j] = 1e30
    for pts in (second, first):
        x.copy_(to_device(torch, pts))
        out.view(torch.int32).fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_host(out), _want(torch, pts, edges, group=3, bucket=8))
    # through the wrapper
    out2 = torch.empty((3, 16382, 17), dtype=torch.uint32, device="cuda")
    graph2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph2):
        ch.level_hist(x, list(edges), group=2, bucket=1, lo=1, hi=16383, out=out2)
    x.copy_(to_device(torch, second))
    out2.view(torch.int32).fill_(-1)
    graph2.replay()
    torch.cuda.synchronize()
    assert torch.equal(_host(out2), _want(torch, second, edges, group=2, bucket=1, lo=1, hi=16383))
    # the form of two operations (a memset of the output and the launch: G x tiles = 64, A = 70) captures and replays as well
    wide = _data(70, edges, 1993)
    x3 = to_device(torch, wide)
    out3 = torch.empty((1, N // 4, 17), dtype=torch.uint32, device="cuda")
    graph3 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph3):
        ch.level_hist(x3, list(edges), bucket=4, out=out3)
    for pts in (wide[::-1], wide * np.float32(2.0)):
        pts = np.ascontiguousarray(pts)
        x3.copy_(to_device(torch, pts))
        out3.view(torch.int32).fill_(-1)
        graph3.replay()
        torch.cuda.synchronize()
        assert torch.equal(_host(out3), _want(torch, pts, edges, group=70, bucket=4))


def _spectra(ch, torch, kind, seed):
    """[4, N] float32 magnitudes on the device: the float chain in mode 0xB1 or 0xA1, or the integer chain's `mag`; and the
    samples they came from"""
    x = to_device(torch, _tones(4, seed))
    if kind == "q15":
        return x, ch.process_q15(x, out_kind="mag")
    if kind == 0xA1:
        ch.load_sos(load_golden("g2_config1.npz")["sos"])
    ch.set_filter_mode(kind)
    return x, ch.process_f32(x, out_kind="mag_full")


@pytest.mark.parametrize("kind", [0xB1, 0xA1, "q15"])
def test_against_the_siblings(ch, torch_mod, kind):
    """With L = 2 and the edge at an order statistic of a row, the row's level-0 total is the number of keys strictly below
    that value; with the edge at the frame's marker peak, level 1 is non-empty exactly in the columns that hold a bin
    attaining the peak."""
    torch = torch_mod
    x, mag = _spectra(ch, torch, kind, 2000)
    host = mag.cpu().numpy()
    keys = host.view(np.uint32) & 0x7FFFFFFF
    for k in (0, 5000, 8191, N - 1):
        stat = ch.order_stats(mag, [k]).cpu().numpy()
        for r in range(4):
            got = _hist(ch, torch, mag[r:r + 1], [float(stat[r, 0])], bucket=16)
            below = int((keys[r] < (int(np.float32(stat[r, 0]).view(np.uint32)) & 0x7FFFFFFF)).sum())
            assert int(got[0, :, 0].sum()) == below and int(got[0, :, 1].sum()) == N - below, (kind, k, r)
    peak_mag = (ch.markers_q15(x) if kind == "q15" else ch.markers(x))[0].cpu().numpy()
    assert (peak_mag > 0).all()
    for r in range(4):
        got = _hist(ch, torch, mag[r:r + 1], [float(peak_mag[r])], bucket=16)
        holds = (host[r] == peak_mag[r]).reshape(N // 16, 16).any(axis=1)
        assert holds.any() and np.array_equal((got[0, :, 1] > 0).numpy(), holds), (kind, r)


def test_persistence_f32(ch, torch_mod):
    """float32, int16 and packed frames: the composed call equals level_hist on process_f32's magnitudes; the same with a
    caller's work and out and at overlap depth 2; wrong arguments are refused before the chain runs."""
    from fpga_real_time_fft_analyzer_amd import frames
    from fpga_real_time_fft_analyzer_amd.abi import SpecanError
    torch = torch_mod
    ch.set_filter_mode(0xB1)
    B = 4
    edges = frames.level_edges_db(2000.0, 80.0, 32)
    forms = _inputs(torch, _tones(B, 2010))
    wants = {}
    for form, x in forms.items():
        m = ch.process_f32(x, out_kind="mag_full")
        wants[form] = _hist(ch, torch, m, edges, bucket=16)
        assert torch.equal(wants[form], _want(torch, m.cpu().numpy(), edges, group=B, bucket=16)), form
        got = ch.persistence_f32(x, edges)
        assert tuple(got.shape) == (1, N // 16, 32) and got.dtype == torch.uint32 and torch.equal(_host(got), wants[form]), form
        per = ch.persistence_f32(x, edges, group=2, bucket=4, lo=1000, hi=3000)
        assert torch.equal(_host(per), _hist(ch, torch, m, edges, group=2, bucket=4, lo=1000, hi=3000)), form
    x = forms["int16"]
    m = ch.process_f32(x, out_kind="mag_full").clone()
    # a caller's work and out
    work = torch.full((B + 1, N), 3.0, dtype=torch.float32, device="cuda")
    out = torch.empty((1, N // 16, 32), dtype=torch.uint32, device="cuda")
    res = ch.persistence_f32(x, edges, work=work, out=out)
    assert res.data_ptr() == out.data_ptr() and torch.equal(_host(out), wants["int16"])
    assert torch.equal(work[:B], m) and (work[B] == 3.0).all().item()
    # overlap depth 2: the input and the workspace dropped and scribbled over right behind the call
    ch.set_overlap(2)
    for form, x2 in forms.items():
        x2, w2 = x2.clone(), torch.empty((B, N), dtype=torch.float32, device="cuda")
        res = ch.persistence_f32(x2, edges, work=w2)
        del x2, w2
        scribble = [torch.full((B, N), 7e7, dtype=torch.float32, device="cuda"), torch.full(x.shape, 85, dtype=x.dtype, device="cuda")]
        torch.cuda.synchronize()
        assert torch.equal(_host(res), wants[form]), form
        res = ch.persistence_f32(forms[form], edges)              # and with the cached workspace
        torch.cuda.synchronize()
        assert torch.equal(_host(res), wants[form]), form
        del scribble
    ch.set_overlap(1)
    # refusals of the composed call, before any launch: the workspace and the out keep what they held
    out.view(torch.int32).fill_(-2)
    for code, kw in ((SA_ESHAPE, dict(group=3)), (SA_EINVAL, dict(group=0)), (SA_EINVAL, dict(bucket=3)), (SA_EINVAL, dict(lo=8, hi=8)),
                     (SA_EINVAL, dict(lo=8)), (SA_EINVAL, dict(edges=[2.0, 1.0])), (SA_EINVAL, dict(edges=[])),
                     (SA_EINVAL, dict(edges=[float("nan")])), (SA_EINVAL, dict(group=2.0)),
                     (SA_ESHAPE, dict(out=torch.empty((1, N // 16, 31), dtype=torch.uint32, device="cuda"))),
                     (SA_ESHAPE, dict(out=torch.empty((1, N // 16, 32), dtype=torch.int32, device="cuda"))),
                     (SA_ESHAPE, dict(work=torch.empty((B - 1, N), dtype=torch.float32, device="cuda")))):
        work.fill_(3.0)
        with pytest.raises(SpecanError) as e:
            ch.persistence_f32(x, **dict(dict(edges=edges, work=work, out=out), **kw))
        torch.cuda.synchronize()
        assert e.value.code == code, kw
        assert (out.view(torch.int32) == -2).all().item() and ("work" in kw or (work == 3.0).all().item()), kw


def test_the_library_is_on_the_map_and_touches_no_other_state(ch, torch_mod):
    torch = torch_mod
    ch.set_filter_mode(0xB1)
    x = to_device(torch, _tones(4, 2020))
    before = ch.process_f32(x, out_kind="mag_full").clone()
    ch.level_hist(before, [1.0, 10.0, 100.0], bucket=16)
    ch.persistence_f32(x, [1.0, 10.0, 100.0])
    assert torch.equal(ch.process_f32(x, out_kind="mag_full"), before)
    assert "libspecan_hist.so" in open("/proc/self/maps").read()
