"""The CFAR normalisation on the device (include/specan_cfar.h, libspecan_cfar.so; SpectrumChain.cfar / cfar_f32) against
frames.cfar_of_rows: every comparison is bit for bit, on every bin, on integer views.

The kernel works a row in 8 tiles of 2048 bins and a thread holds quads 1024 bins apart: every full-range case has windows
across each of those seams, and the ranges with odd ends cut through the first and the last tile."""
import itertools

import numpy as np
import pytest

from conftest import N, load_golden
from gpu_support import ch, check_overlap_profiling_and_graph_capture, lds_fill, to_device, torch_mod  # noqa: F401 (fixtures)
from test_f32_cfar_cpu import FIELDS, INF, MODES, QNAN, WHATS, bits, random_rows, records_of, shaped_rows, special_rows
from test_gpu_f32_peaks import _inputs, _tones

pytestmark = pytest.mark.gpu

SA_OK, SA_EINVAL, SA_ESHAPE = 0, -1, -2
# (train, guard, lo, hi): the ends of both parameters and the defaults on the full row; odd ends near both ends of the row;
# a range inside one tile, one that ends on a tile seam and one that is as narrow as the guard allows
SETUPS = ((1, 0, 0, N), (64, 64, 0, N), (16, 2, 0, N), (4, 1, 1, N - 1), (8, 3, 37, 16001), (32, 7, 1023, 2051), (64, 64, 2047, 2177),
          (2, 0, 16381, N), (64, 5, 3, 4096), (1, 64, 2049, 16383))


def _check(ch, torch, x, pts, field, tag, **kw):
    """ch.cfar on the device tensor `x` equals the mirror on `pts`, on every bin"""
    from fpga_real_time_fft_analyzer_amd import frames
    got = ch.cfar(x, field=field, **kw).view(torch.int32).cpu().numpy().view(np.uint32)
    want = bits(frames.cfar_of_rows(records_of(pts, field), field=field, **kw))
    assert got.shape == want.shape and np.array_equal(got, want), (tag, kw, np.argwhere(got != want)[:5].tolist(),
                                                                   int((got != want).sum()))
    return want


@pytest.mark.parametrize("field", FIELDS)
def test_random_rows_equal_the_mirror(ch, torch_mod, field):
    """Wide-range rows, noise with signs and small integers: each mode and output on every setup, every bin."""
    pts = random_rows()
    x = to_device(torch_mod, records_of(pts, field))
    for (train, guard, lo, hi), mode, what in itertools.product(SETUPS, MODES, WHATS):
        want = _check(ch, torch_mod, x, pts, field, "random", train=train, guard=guard, mode=mode, what=what, lo=lo, hi=hi)
        assert want[:, lo:hi].any() and not want[:, :lo].any() and not want[:, hi:].any()


def test_specials_equal_the_mirror(ch, torch_mod):
    """NaNs in a window and as the point, +inf, -0.0, denormals, the all-zero row and the denormal ratio: the mirror's bits,
    and the one NaN pattern."""
    pts = special_rows()
    infinite = set()                                           # the calls whose result holds an infinity: some of every output
    for field in FIELDS:
        x = to_device(torch_mod, records_of(pts, field))
        for mode, what, (train, guard) in itertools.product(MODES, WHATS, ((4, 1), (1, 0), (64, 3))):
            want = _check(ch, torch_mod, x, pts, field, "specials", train=train, guard=guard, mode=mode, what=what)
            nan = np.isnan(want.view(np.float32))
            assert nan.any() and (want[nan] == QNAN).all()
            if (want == INF).any():
                infinite.add(what)
    assert infinite == set(WHATS)
    den = _check(ch, torch_mod, to_device(torch_mod, records_of(pts, "power")), pts, "power", "denormal", train=4, guard=1)[5, 5000]
    assert 0 < den < 0x00800000


def test_known_answers_of_the_header(ch, torch_mod):
    torch = torch_mod
    x = torch.ones((3, N), dtype=torch.float32, device="cuda")
    x[1, 100] = 3.0
    at = [0, 97, 98, 99, 100, 101, 102, N - 1]
    want = {"ca": [1.0, 0.5, 0.5, 1.0, 9.0, 1.0, 0.5, 1.0], "go": [1.0, 1 / 3, 1 / 3, 1.0, 9.0, 1.0, 1 / 3, 1.0], "so": [1.0] * 4 + [9.0] + [1.0] * 3}
    for mode in MODES:
        got = ch.cfar(x, 4, 1, mode)
        assert got[1, at].view(torch.int32).tolist() == bits(np.array(want[mode], np.float32)).view(np.int32).tolist(), mode
        assert (got[0] == 1.0).all().item() and (got[2] == 1.0).all().item(), mode
    assert ch.cfar(x, 4, 1, "go")[1, 97].view(torch.int32).item() == 0x3EAAAAAB


def test_exactly_the_output_bytes_are_written_and_a_refused_call_writes_nothing(ch, torch_mod):
    from fpga_real_time_fft_analyzer_amd import abi, frames
    from fpga_real_time_fft_analyzer_amd.abi import SpecanError
    torch = torch_mod
    L = abi.cfar_lib()
    stream = torch.cuda.current_stream().cuda_stream
    pts = random_rows()
    R, guard = 4, 4096
    x = to_device(torch, pts)
    for kw in (dict(log2_train=4, guard=2, mode=0, what=0, lo=0, hi=N), dict(log2_train=6, guard=64, mode=1, what=1, lo=37, hi=16001),
               dict(log2_train=0, guard=0, mode=2, what=0, lo=8000, hi=8002)):
        for fill in (0xFF, 0x00):
            buf = torch.full((guard + R * N * 4 + guard,), fill, dtype=torch.uint8, device="cuda")
            assert L.sa_cfar_f32(x.data_ptr(), 0, buf.data_ptr() + guard, R, kw["log2_train"], kw["guard"], kw["mode"], kw["what"],
                                 kw["lo"], kw["hi"], stream) == SA_OK
            assert L.sa_cfar_last_error() == b""
            torch.cuda.synchronize()
            assert (buf[:guard] == fill).all().item() and (buf[guard + R * N * 4:] == fill).all().item()
            got = buf[guard:guard + R * N * 4].cpu().numpy().view(np.uint32).reshape(R, N)
            want = bits(frames.cfar_of_rows(pts, 1 << kw["log2_train"], kw["guard"], MODES[kw["mode"]], WHATS[kw["what"]], kw["lo"], kw["hi"]))
            assert np.array_equal(got, want), (kw, fill)                   # every float stored: the fill shows nowhere
    # refused calls: the code of sa_cfar_check for the same arguments, its text, and nothing written
    buf = torch.full((R * N * 4 + guard,), 0xFF, dtype=torch.uint8, device="cuda")
    flat = torch.zeros((2 * R * N + 64,), dtype=torch.float32, device="cuda")
    before = flat.clone()
    p_in, p_out = flat.data_ptr(), buf.data_ptr()
    good = dict(field=0, rows=R, log2_train=4, guard=2, mode=0, what=0, lo=0, hi=N)
    good.update({"in": p_in, "out": p_out})
    for tag, kw, code, words in (
            ("in 4 bytes off", {"in": p_in + 4}, SA_EINVAL, "`in` must be 16-byte aligned"),
            ("out 8 bytes off", dict(out=p_out + 8), SA_EINVAL, "`out` must be 16-byte aligned"),
            ("out inside in", dict(out=p_in + R * N * 4 - 16), SA_EINVAL, "`out` (262144 bytes) and `in` (262144 bytes) overlap"),
            ("records read twice as much", dict(field=2, out=p_in + R * N * 4), SA_EINVAL, "`in` (524288 bytes) overlap"),
            ("in place", dict(out=p_in), SA_EINVAL, "overlap"),
            ("NULL out", dict(out=0), SA_EINVAL, "NULL"), ("NULL in", {"in": 0}, SA_EINVAL, "NULL"),
            ("field 3", dict(field=3), SA_EINVAL, "field"), ("mode 3", dict(mode=3), SA_EINVAL, "mode"), ("what 2", dict(what=2), SA_EINVAL, "what"),
            ("log2_train 7", dict(log2_train=7), SA_EINVAL, "log2_train"), ("guard 65", dict(guard=65), SA_EINVAL, "guard"),
            ("range", dict(lo=5, hi=5), SA_EINVAL, "range"), ("narrow", dict(lo=5, hi=10), SA_EINVAL, "2 * guard + 2"),
            ("negative rows", dict(rows=-1), SA_ESHAPE, "negative")):
        a = dict(good, **kw)
        args = (a["rows"], a["log2_train"], a["guard"], a["mode"], a["what"], a["lo"], a["hi"])
        assert L.sa_cfar_check(a["field"], a["in"], a["out"], *args) == code, tag
        assert L.sa_cfar_f32(a["in"], a["field"], a["out"], *args, stream) == code, tag
        assert words in L.sa_cfar_last_error().decode(), (tag, L.sa_cfar_last_error())
    torch.cuda.synchronize()
    assert (buf == 0xFF).all().item() and torch.equal(flat, before)
    assert L.sa_cfar_f32(0, 0, 0, 0, 4, 2, 0, 0, 0, N, stream) == SA_OK and L.sa_cfar_last_error() == b""
    # the buffers touching: in | out in a row
    packed = torch.zeros((2 * R * N,), dtype=torch.float32, device="cuda")
    packed[:R * N] = x.view(-1)
    base = packed.data_ptr()
    assert L.sa_cfar_f32(base, 0, base + R * N * 4 - 16, R, 4, 2, 0, 0, 0, N, stream) == SA_EINVAL
    assert L.sa_cfar_f32(base, 0, base + R * N * 4, R, 4, 2, 0, 0, 0, N, stream) == SA_OK
    torch.cuda.synchronize()
    assert np.array_equal(packed[R * N:].view(torch.int32).cpu().numpy().view(np.uint32).reshape(R, N), bits(frames.cfar_of_rows(pts)))
    assert torch.equal(packed[:R * N], x.view(-1))
    # through the wrapper: shapes and dtypes before any device call
    for code, args, kw in ((SA_ESHAPE, (x[:, :N // 2],), {}), (SA_EINVAL, (x.double(),), {}), (SA_ESHAPE, (x,), dict(field="peak")),
                           (SA_ESHAPE, (x,), dict(out=torch.empty((R, N - 1), dtype=torch.float32, device="cuda"))),
                           (SA_ESHAPE, (x,), dict(out=torch.empty((R, N), dtype=torch.int32, device="cuda"))),
                           (SA_ESHAPE, (x,), dict(out=torch.empty((R, N), dtype=torch.float32))),
                           (SA_EINVAL, (x,), dict(train=3)), (SA_EINVAL, (x,), dict(guard=65)), (SA_EINVAL, (x,), dict(mode="xx")),
                           (SA_EINVAL, (x,), dict(out=x)), (SA_EINVAL, (x.cpu(),), {})):
        with pytest.raises(SpecanError) as e:
            ch.cfar(*args, **kw)
        assert e.value.code == code, (args[0].shape, kw)
    assert tuple(ch.cfar(torch.empty((0, N), dtype=torch.float32, device="cuda")).shape) == (0, N)


def test_poisoned_lds(ch, torch_mod, lds_fill):
    """lds_fill(P) with P = 0xFFFFFFFF (a NaN as either half of a double), 0x7FF00000 (an infinity as the high half) and 0,
    then the call on the same stream: the bits of the mirror, where any entry read before it is written would show."""
    pts = random_rows()
    cases = [dict(train=t, guard=g, mode=m, what=w, lo=lo, hi=hi)
             for (t, g, lo, hi), (m, w) in zip(SETUPS, itertools.cycle(itertools.product(MODES, WHATS)))]
    for field in FIELDS:
        x = to_device(torch_mod, records_of(pts, field))
        for n, kw in enumerate(cases):
            for word in (0xFFFFFFFF, 0x7FF00000, 0):
                if field is not None and (n + (word & 1)) % 2:     # the record layouts take every other case
                    continue
                lds_fill(word)
                _check(ch, torch_mod, x, pts, field, (field, hex(word)), **kw)


def test_capture_and_replay(ch, torch_mod):
    """cfar captures without a warm-up -- it is one launch with its parameters in the launch's arguments -- and two replays
    on different inputs each give the result of their own input."""
    from fpga_real_time_fft_analyzer_amd import frames
    torch = torch_mod
    first = random_rows()
    x = to_device(torch, first)
    out = torch.zeros((4, N), dtype=torch.float32, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ch.cfar(x, 8, 3, "go", "ratio", 37, 16001, out=out)
    seen = []
    for pts in (np.ascontiguousarray(first[::-1]) * np.float32(3.0), first):
        x.copy_(to_device(torch, pts))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got = out.view(torch.int32).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, bits(frames.cfar_of_rows(pts, 8, 3, "go", "ratio", 37, 16001)))
        seen.append(got)
    assert not np.array_equal(seen[0], seen[1])
    assert "libspecan_cfar.so" in open("/proc/self/maps").read()


@pytest.mark.parametrize("mode", [0xB1, 0xA1])
def test_cfar_f32(ch, torch_mod, mode):
    """The composed call at B = 4 equals cfar on process_f32's magnitudes, and with group = 2 cfar on spectra_f32's records,
    field 'power' -- float32, int16 and packed input; overlap, profiling and capture; a caller's work and out; refusals
    before any launch."""
    from fpga_real_time_fft_analyzer_amd import frames
    from fpga_real_time_fft_analyzer_amd.abi import SpecanError
    torch = torch_mod
    if mode == 0xA1:
        ch.load_sos(load_golden("g2_config1.npz")["sos"])
    ch.set_filter_mode(mode)
    B = 4
    tones = _tones(B, 2640 + mode, bins=(1200, 2400, 3600), amps=(900.0, 450.0, 220.0))
    calls = (dict(), dict(train=64, guard=8, mode="go", what="floor", lo=101, hi=9001), dict(train=4, guard=1, mode="so"))
    for form, x in _inputs(torch, tones).items():
        mag = ch.process_f32(x, out_kind="mag_full").clone()
        rec2 = ch.spectra_f32(x, 2).clone()
        for (t, field, group), kw in itertools.product(((mag, None, None), (rec2, "power", 2)), calls):
            want = ch.cfar(t, field=field, **kw)
            got = torch.zeros((t.shape[0], N), dtype=torch.float32, device="cuda")
            ret = ch.cfar_f32(x, group=group, out=got, **kw)
            assert ret.data_ptr() == got.data_ptr() and torch.equal(got.view(torch.int32), want.view(torch.int32)), (form, group, kw)
            mirror = bits(frames.cfar_of_rows(t.cpu().numpy(), field=field, **kw))
            assert np.array_equal(got.view(torch.int32).cpu().numpy().view(np.uint32), mirror), (form, group, kw)
        # the three tones stand far above their local floor: by A^2 N / (4 sigma^2), some 10^5, where the noise is the floor
        ratio = ch.cfar_f32(x)
        assert tuple(ratio.shape) == (B, N) and (ratio[:, [1200, 2400, 3600]] > 50.0).all().item(), form
    x = _inputs(torch, tones)["int16"]
    mag = ch.process_f32(x, out_kind="mag_full").clone()
    ref = ch.cfar(mag, 16, 2, "go").clone()
    ch.cfar_f32(x, 16, 2, "go")                                                # the cached workspace, before the capture
    check_overlap_profiling_and_graph_capture(torch, ch, lambda o: ch.cfar_f32(x, 16, 2, "go", out=o), ref)
    work = torch.full((B + 1, N), 3.0, dtype=torch.float32, device="cuda")
    got = ch.cfar_f32(x, 16, 2, "go", work=work)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32)) and torch.equal(work[:B], mag) and (work[B] == 3.0).all().item()
    for code, args, kw in ((SA_ESHAPE, (x[:3],), dict(group=2)), (SA_EINVAL, (x,), dict(group=3)), (SA_EINVAL, (x,), dict(train=5)),
                           (SA_EINVAL, (x,), dict(guard=65)), (SA_EINVAL, (x,), dict(mode="og")), (SA_EINVAL, (x,), dict(what="db")),
                           (SA_EINVAL, (x,), dict(lo=0, hi=5)),
                           (SA_ESHAPE, (x,), dict(work=torch.empty((B - 1, N), dtype=torch.float32, device="cuda"))),
                           (SA_ESHAPE, (x,), dict(out=torch.zeros((B, N - 1), dtype=torch.float32, device="cuda"))),
                           (SA_ESHAPE, (x,), dict(group=2, out=torch.zeros((B, N), dtype=torch.float32, device="cuda")))):
        work.fill_(3.0)
        with pytest.raises(SpecanError) as e:
            ch.cfar_f32(*args, **dict(dict(work=work), **kw))
        torch.cuda.synchronize()
        assert e.value.code == code and (work == 3.0).all().item(), kw


def test_the_ratio_feeds_the_signal_list(ch, torch_mod):
    """The use the feature is for, on the device: find_signals on cfar's ratio, with cfar_alpha as the threshold, equals
    signals_of_rows on the mirror's ratio -- exactly the planted tones -- where six times the row's median on the raw rows is
    blind to them and reports segments by the hundred."""
    from fpga_real_time_fft_analyzer_amd import frames
    from test_f32_signals_cpu import same_result
    torch = torch_mod
    mag, tones = shaped_rows()
    x = to_device(torch, mag)
    alpha = frames.cfar_alpha(1e-6, 32)
    ratio = ch.cfar(x, 16, 2, "ca", "ratio")
    bounds, peak, peak_bin, power, stats = ch.find_signals(ratio, 32, alpha)
    mirror = frames.cfar_of_rows(mag, 16, 2, "ca", "ratio")
    want = frames.signals_of_rows(mirror, k=32, threshold=alpha)
    rec = np.zeros((4, 32), frames.SIGNAL)
    rec["start"], rec["stop"] = bounds[..., 0].cpu().numpy(), bounds[..., 1].cpu().numpy()
    rec["peak"], rec["peak_bin"], rec["power"] = peak.cpu().numpy(), peak_bin.cpu().numpy(), power.cpu().numpy()
    assert same_result((rec, stats.cpu().numpy()), want) is None
    assert stats[:, 0].tolist() == [5] * 4 and bounds[:, :5, 0].tolist() == tones
    raw = ch.find_signals(x, 32, to_device(torch, (np.float32(6.0) * np.median(mag, axis=1)).astype(np.float32)))
    assert (raw[4][:, 0] >= 200).all().item() and not np.isin(raw[0][..., 0].cpu().numpy(), np.array(tones).ravel()).any()
