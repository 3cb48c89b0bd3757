"""GPU: stream ordering of the host side, tested against a GPU that lags behind the host.

Every other test reads a result back (or synchronises) before the next setter or buffer reuse, or uses batches so small
that the kernel is over before Python reaches the next line.  A missing stream wait in the library's upload / call
ordering, or a feeder that recycles a buffer too early, passes all of that.  Here a stream is HELD: tests/hip/stream_hold.hip
(built by the fixture below, loaded with ctypes; not part of the library) parks one wave on it for a bounded time, so
whatever is not ordered behind the held work is certain to overtake it.

  - premise: the hold lasts as long as asked; an event behind it is pending; pick_held_stream() finds a stream whose
    hold does not also hold the streams that must stay free (the runtime maps streams onto four hardware queues, and two
    streams on one queue run in order: that would hide every defect looked for here).
  - every held scenario checks, right after its last enqueue, that the hold had not ended (the vacuity check), and
    prints the host time its enqueues took against the hold H.
  - part 2: ingest.DeviceFeeder under a model consumer that follows the overlap contract of include/specan.h with torch
    streams and a hold in front of every read.  Deterministic.
  - part 3: the feeder with the real chain at overlap depths 1..3 (nothing can be held there).
  - part 4: trains of control-plane states and process calls behind a hold, no host synchronisation inside a train.
  - part 5: a joined result is visible on the caller's stream (a race by nature: see the test).

Streams of this module: the caller's stream, a second free one, at most 8 hold candidates (usually three or four are
made) and one copy stream per cached feeder.  Every hold is one wave and at most HOLD_MS long; the module's holds add up
to a few seconds (the last test prints and bounds the sum)."""
import ctypes
import itertools
import time

import numpy as np
import pytest

from conftest import N, load_golden
from gpu_support import torch_mod  # noqa: F401 (fixtures)
from native import exported, gpu_helper
from structured_cases import cascades

HOLD_MS = 40               # H of every held scenario; the enqueues it has to outlast took 0.04 .. 0.74 ms (FIGURE lines)
PROBE_MS = 20              # the hold of pick_held_stream
FREE_WITHIN_S = 5e-3       # ... within which work on a free stream must complete
MAX_CANDIDATES = 8
P12_ROW = 3 * N // 2
SIZES = (8, 8, 5, 8, 1, 8, 8, 3)          # frames per batch of the feeder tests, max_batch = 8


# --------------------------------------------------------------------------------------------------- the hold helper
@pytest.fixture(scope="module")
def hold_so(tmp_path_factory):
    return gpu_helper(tmp_path_factory.mktemp("stream_hold"), "stream_hold")


def test_stream_hold_cross_compiles(hold_so):
    """CPU: the helper builds for gfx950 and exports its one C entry point."""
    assert "stream_hold" in exported(hold_so)


class Env:
    """The module's streams and the hold.  `main` is the caller's stream of the feeder tests; `free` a second stream."""

    def __init__(self, so, torch):
        self.torch = torch
        L = ctypes.CDLL(so)                    # torch is imported: the helper binds to the HIP runtime torch mapped
        L.stream_hold.argtypes = [ctypes.c_uint, ctypes.c_void_p]
        L.stream_hold.restype = ctypes.c_int
        self.L = L
        self.held_ms = 0                       # sum of all holds enqueued
        self.main = torch.cuda.Stream()
        self.free = torch.cuda.Stream()
        self._candidates = []
        self.small_pin = torch.arange(1024, dtype=torch.int32).pin_memory()
        self.small_dev = torch.zeros(1024, dtype=torch.int32, device="cuda")
        self.hold_raw(0, self.main)            # the helper's code object is loaded before anything is timed
        torch.cuda.synchronize()

    def hold_raw(self, ms, stream):
        return self.L.stream_hold(ms, stream.cuda_stream)

    def hold(self, ms, stream):
        """Hold `stream` for `ms`; the event recorded behind the hold."""
        rc = self.hold_raw(ms, stream)
        assert rc == 0, f"stream_hold: hipError {rc}"
        self.held_ms += ms
        ev = self.torch.cuda.Event()
        ev.record(stream)
        return ev

    def candidates(self):
        """Fresh streams, made as they are asked for, MAX_CANDIDATES in the life of the module."""
        i = 0
        while i < MAX_CANDIDATES:
            if i == len(self._candidates):
                self._candidates.append(self.torch.cuda.Stream())
            yield self._candidates[i]
            i += 1


@pytest.fixture(scope="module")
def env(hold_so, hip_lib_built, torch_mod):
    return Env(hold_so, torch_mod)


def _completes_within(ev, seconds):
    """Poll `ev` (no sleep, no host wait that could outlast the hold): True as soon as it has completed."""
    t_end = time.perf_counter() + seconds
    while time.perf_counter() < t_end:
        if ev.query():
            return True
    return ev.query()


def pick_held_stream(env, must_stay_free, taken=(), extra=None):
    """The first candidate stream on which a PROBE_MS hold delays neither a small pinned-to-device copy on each stream of
    `must_stay_free` nor `extra(end_event)` (a probe of the caller's own: True = not delayed).  Candidates in `taken` are
    passed over.  No candidate: the tests that asked would pass vacuously, so they fail."""
    torch = env.torch
    tried = []
    for cand in env.candidates():
        if any(cand is t for t in taken) or any(cand is s for s in must_stay_free):
            continue
        torch.cuda.synchronize()
        end = env.hold(PROBE_MS, cand)
        ok = True
        for s in must_stay_free:
            ev = torch.cuda.Event()
            with torch.cuda.stream(s):
                env.small_dev.copy_(env.small_pin, non_blocking=True)
                ev.record(s)
            ok = _completes_within(ev, FREE_WITHIN_S) and not end.query()
            if not ok:
                break
        if ok and extra is not None:
            ok = bool(extra(end)) and not end.query()
        end.synchronize()
        tried.append((hex(cand.cuda_stream), ok))
        if ok:
            print(f"FIGURE held stream picked: {hex(cand.cuda_stream)} after {len(tried)} candidate(s); kept free: "
                  f"{[hex(s.cuda_stream) for s in must_stay_free]}{' + the probe' if extra else ''}")
            return cand
    pytest.fail(f"hold premise NOT met: every candidate stream {tried} shares a hardware queue with a stream that must "
                f"stay free while it is held.  A hold would then delay the very operation whose missing ordering the "
                f"test looks for, so every ordering test that asked for this stream would pass vacuously.")


def _vacuity(env, end, t0, what, hold_ms=HOLD_MS):
    """Right after the last enqueue of a held part: the hold must still be pending, or the test has shown nothing."""
    dt = time.perf_counter() - t0
    pending = not end.query()
    print(f"FIGURE enqueue {what}: {dt * 1e3:.3f} ms of host time under a hold of {hold_ms} ms")
    assert pending, f"{what}: the hold ended before the enqueues did ({dt * 1e3:.3f} ms): nothing was tested"
    assert 4 * dt * 1e3 <= hold_ms, f"{what}: the hold is less than four times the enqueues' {dt * 1e3:.3f} ms"
    return dt


# ----------------------------------------------------------------------------------------------------- part 1: premise
@pytest.mark.gpu
def test_hold_refuses_more_than_100_ms(env, torch_mod):
    torch_mod.cuda.synchronize()
    ev = torch_mod.cuda.Event()
    assert env.hold_raw(101, env.main) != 0 and env.hold_raw(100000, env.main) != 0
    ev.record(env.main)
    assert _completes_within(ev, 1.0)                     # nothing was launched: the stream is idle


@pytest.mark.gpu
def test_hold_lasts_as_long_as_asked(env, torch_mod):
    """Between events recorded around a hold of H = 10 and 40 ms: at least 0.9 H (the counter has a constant rate), at
    most 3 H (the iteration cap, were it what ends the wait, must not be far above the counter's limit); and an event
    recorded behind a hold is pending right after the enqueue.  Measured: 10.005 ms and 40.007 ms."""
    for H in (10, 40):
        torch_mod.cuda.synchronize()
        a = torch_mod.cuda.Event(enable_timing=True)
        b = torch_mod.cuda.Event(enable_timing=True)
        a.record(env.main)
        assert env.hold_raw(H, env.main) == 0
        env.held_ms += H
        b.record(env.main)
        pending = not b.query()
        b.synchronize()
        ms = a.elapsed_time(b)
        print(f"FIGURE hold of {H} ms lasted {ms:.3f} ms")
        assert pending, "the event behind the hold had completed right after the enqueue"
        assert 0.9 * H <= ms <= 3.0 * H, (H, ms)


@pytest.mark.gpu
def test_a_held_stream_leaves_a_free_one_running(env, torch_mod):
    """pick_held_stream finds a stream whose hold delays neither the module's caller stream nor its second stream."""
    s = pick_held_stream(env, [env.main, env.free])
    assert s is not env.main and s is not env.free


# ------------------------------------------------------------------------------- part 2: feeder under a model consumer
def _batches(packed, seed, sizes=SIZES):
    rng = np.random.default_rng(seed)
    if packed:
        return [rng.integers(0, 256, (n, P12_ROW), dtype=np.uint8) for n in sizes]
    return [rng.integers(-32768, 32768, (n, N)).astype(np.int16) for n in sizes]


_FEEDERS = {}


def _feeder(packed, depth):
    """One feeder per (packed, depth) for the module: its copy stream is one more stream of the process."""
    from fpga_real_time_fft_analyzer_amd.ingest import DeviceFeeder
    key = (bool(packed), depth)
    if key not in _FEEDERS:
        _FEEDERS[key] = DeviceFeeder(0, max_batch=8, packed=packed, consumer_depth=depth)
    return _FEEDERS[key]


_SIDES = {}


def _side_streams(env, feeder, depth):
    """depth streams that can be held while the feeder's copy stream and the caller's stream go on."""
    key = id(feeder)
    if key not in _SIDES:
        sides = []
        for _ in range(depth if depth > 1 else 0):
            sides.append(pick_held_stream(env, [feeder._copy_stream, env.main], taken=sides))
        _SIDES[key] = sides
    return _SIDES[key]


class ModelConsumer:
    """The overlap contract of include/specan.h to the letter, with torch streams.  Call k at depth d: side stream k % d
    waits for the current stream (the fork); the current stream waits for the `done` event of slot (k + 1) % d if that
    slot is unjoined (the join); on the side stream: hold, out[k] <- x, record `done`.  Depth 1: the same work on the
    current stream itself.  Each call checks that its own read is still pending when it returns (the vacuity check)."""

    def __init__(self, env, depth, sides, out):
        self.env, self.d, self.sides, self.out = env, depth, sides, out
        self.cur = env.main
        ev = env.torch.cuda.Event
        self.fork = [ev() for _ in range(depth)]
        self.done = [ev() for _ in range(depth)]
        self.unjoined = [False] * depth
        self.k = 0
        self.worst_enqueue = 0.0

    def __call__(self, x):
        torch, k, d = self.env.torch, self.k, self.d
        slot = k % d
        t0 = time.perf_counter()
        if d == 1:
            side = self.cur
        else:
            side = self.sides[slot]
            self.fork[slot].record(self.cur)
            j = (k + 1) % d
            if self.unjoined[j]:
                self.cur.wait_event(self.done[j])
                self.unjoined[j] = False
            side.wait_event(self.fork[slot])
        self.env.hold(HOLD_MS, side)
        with torch.cuda.stream(side):
            self.out[k, :x.shape[0]].copy_(x)
            self.done[slot].record(side)
        self.unjoined[slot] = d > 1
        dt = time.perf_counter() - t0
        pending = not self.done[slot].query()
        self.worst_enqueue = max(self.worst_enqueue, dt)
        assert pending, f"call {k}: the held read had run {dt * 1e3:.3f} ms after its enqueue began: nothing was tested"
        self.k += 1

    def flush(self):
        for j in range(self.d):
            if self.unjoined[j]:
                self.cur.wait_event(self.done[j])
                self.unjoined[j] = False


def _model_run(env, packed, depth, feeds, seed):
    """`feeds`: [(sizes, take)]: feed() batches of those sizes and let the consumer take `take` of them (None: all), then
    flush.  Every batch taken must arrive in its `out` row bit for bit."""
    torch = env.torch
    feeder = _feeder(packed, depth)
    sides = _side_streams(env, feeder, depth)
    total = sum(len(s) if t is None else t for s, t in feeds)
    out = torch.zeros((total, 8, feeder._row), dtype=torch.uint8 if packed else torch.int16, device="cuda")
    torch.cuda.synchronize()
    taken = []
    with torch.cuda.stream(env.main):
        cons = ModelConsumer(env, depth, sides, out)
        for f, (sizes, take) in enumerate(feeds):
            bs = _batches(packed, seed + f, sizes)
            for i, x in enumerate(feeder.feed(iter(bs))):
                cons(x)
                taken.append(bs[i])
                if take is not None and i + 1 == take:
                    break
            cons.flush()
    torch.cuda.synchronize()
    print(f"FIGURE model consumer packed={packed} depth={depth}: worst enqueue {cons.worst_enqueue * 1e3:.3f} ms per "
          f"call under a hold of {HOLD_MS} ms; side streams {[hex(s.cuda_stream) for s in sides]}")
    assert 4 * cons.worst_enqueue * 1e3 <= HOLD_MS
    got = out.cpu().numpy()
    bad = [k for k, b in enumerate(taken) if not np.array_equal(got[k, :b.shape[0]], b)]
    assert not bad, f"batches {bad} of {len(taken)} did not reach the consumer as they were fed"


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("packed", [False, True], ids=["int16", "packed"])
def test_feeder_keeps_a_batch_until_the_consumer_has_read_it(env, packed, depth):
    """8 ragged batches through a consumer whose reads lag its calls by a 40 ms hold and, at depth d > 1, are joined d-1
    calls late.  Measured: the enqueues of a call took 0.04 .. 0.14 ms of host time (the worst call of each run), against
    H = 40 ms; the test asks for H >= 4 x that figure."""
    _model_run(env, packed, depth, [(SIZES, None)], seed=100 + depth)


@pytest.mark.gpu
def test_feeder_two_feeds_in_a_row(env):
    """The second feed() must not rewrite what the last calls of the first one, joined only by the flush, still read."""
    _model_run(env, False, 2, [((8, 3, 8), None), ((5, 8, 8), None)], seed=200)


@pytest.mark.gpu
def test_feeder_after_an_abandoned_feed(env):
    """The consumer stops after 3 of 5 batches (one more is already copied and never handed out), flushes, and feeds anew."""
    _model_run(env, False, 2, [((8, 8, 5, 8, 8), 3), ((8, 1, 8, 3), None)], seed=300)


@pytest.mark.gpu
def test_feeder_refusals(env):
    from fpga_real_time_fft_analyzer_amd.ingest import DeviceFeeder
    for d in (0, 5):
        with pytest.raises(ValueError):
            DeviceFeeder(0, max_batch=8, consumer_depth=d)
    feeder = _feeder(False, 1)
    bs = _batches(False, 7, (2, 2, 2))
    with env.torch.cuda.stream(env.main):
        old = feeder.feed(iter(bs))
        next(old)
        assert sum(1 for _ in feeder.feed(iter(bs))) == 3
        with pytest.raises(RuntimeError):
            next(old)
        with pytest.raises(ValueError):
            list(feeder.feed(iter([np.zeros((9, N), np.int16)])))
    env.torch.cuda.synchronize()


# ------------------------------------------------------------------------------------ part 3: feeder with the real chain
G2 = load_golden("g2_config1.npz")["sos"]


def _chain_paths():
    from fpga_real_time_fft_analyzer_amd.ingest import pack12
    rng = np.random.default_rng(31)
    b16 = [rng.integers(-2048, 2048, (n, N)).astype(np.int16) for n in SIZES]

    def q15(c):
        c.set_filter_mode(0x00)
        return c.process_q15

    def f32(c):
        c.load_sos(G2)
        c.set_filter_mode(0xA1)
        return c.process_f32

    return {"q15": (q15, False, b16), "f32_i16": (f32, False, b16), "f32_p12": (f32, True, [pack12(b) for b in b16])}


_CHAIN_REFS = {}


def _chain_ref(chain_cls, torch, path):
    """The batches one by one on a fresh ordered handle, each read back before the next."""
    if path not in _CHAIN_REFS:
        setup, _, bs = _chain_paths()[path]
        c = chain_cls(0)
        call = setup(c)
        _CHAIN_REFS[path] = [call(torch.from_numpy(b).cuda()).cpu() for b in bs]
        c.close()
    return _CHAIN_REFS[path]


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("path", ["q15", "f32_i16", "f32_p12"])
def test_feeder_with_the_real_chain(env, chain_cls, torch_mod, path, depth):
    """The chain at overlap depth d behind a feeder of consumer_depth d, results held as tensors, one flush at the end:
    bit for bit what a fresh ordered handle gives batch by batch."""
    setup, packed, bs = _chain_paths()[path]
    ref = _chain_ref(chain_cls, torch_mod, path)
    c = chain_cls(0)
    try:
        with torch_mod.cuda.stream(env.main):
            call = setup(c)
            c.set_overlap(depth)
            outs = [call(xd) for xd in _feeder(packed, depth).feed(iter(bs))]
            c.flush()
        torch_mod.cuda.synchronize()
        bad = [k for k in range(len(bs)) if not torch_mod.equal(outs[k].cpu(), ref[k])]
        assert not bad, f"batches {bad} differ from the ordered handle's results"
    finally:
        c.close()


# ------------------------------------------------------------- part 4: control-plane uploads behind pending launches
B4 = 4
FORMS = ("ordered", "alternating", "overlap2", "overlap3")


@pytest.fixture(scope="module")
def plane(env, chain_cls, torch_mod):
    """(handle, held stream S, free stream F) for the trains.  S is picked so that holding it holds neither F nor the
    handle's control stream, which the test cannot name: with the handle idle and S held, a table-uploading setter and
    then a process call on F must complete while the hold is pending."""
    torch = torch_mod
    c = chain_cls(0)
    F = env.free
    x = torch.from_numpy(np.random.default_rng(5).integers(-2048, 2048, (B4, N)).astype(np.int16)).cuda()
    out = torch.empty((B4, N, 2), dtype=torch.int16, device="cuda")
    rom = c.window_q15()
    with torch.cuda.stream(F):
        c.set_window_q15(rom)
        c.process_q15(x, out)                  # code objects loaded, workspaces grown
    torch.cuda.synchronize()

    def control_stream_is_free(end):
        ev = torch.cuda.Event()
        c.set_window_q15(rom)
        with torch.cuda.stream(F):
            c.process_q15(x, out)
            ev.record(F)
        return _completes_within(ev, FREE_WITHIN_S)

    S = pick_held_stream(env, [F], extra=control_stream_is_free)
    yield c, S, F
    c.close()


def _reset(c):
    c.set_overlap(1)
    c.set_precision("f32")
    c.set_filter_mode(0xB1)
    c.set_window_f32(None)
    c.set_window_q15(None)
    c.set_window_mode_q15(0)
    c.set_marker_range(0, N)


def _x_f32(torch):
    x = 0.3 * np.random.default_rng(41).standard_normal((B4, N))
    x[0] = 0.0
    x[0, 0] = 1.0
    return torch.from_numpy(x.astype(np.float32)).cuda()


def _x_i16(torch):
    return torch.from_numpy(np.random.default_rng(42).integers(-2048, 2048, (B4, N)).astype(np.int16)).cuda()


def _hamming():
    """0.54 - 0.46 cos(2 pi n / (N-1)): the library fits it and generates it in place (no window table read)."""
    return np.hamming(N).astype(np.float32)


def _blackman():
    return np.blackman(N).astype(np.float32)     # two cosine terms: a table window


def _roms():
    rng = np.random.default_rng(43)
    return [None] + [rng.integers(-32768, 32768, N).astype(np.int16) for _ in range(3)]


def _pairs(states):
    """A cycle of states as trains of two: for setters that fill the staging ring (4 uploads) on their own."""
    return [[states[i], states[(i + 1) % len(states)]] for i in range(len(states))]


def _train_lane(c, torch):
    """Custom lane table in 0xA1: load_sos / load_sos_f32 alternating over cascades of 2, 4, 6 (and 6) padded sections;
    one upload per state, three behind the hold."""
    cs = cascades()
    c.set_filter_mode(0xA1)
    x = _x_f32(torch)
    states = [lambda: c.load_sos(cs["long_memory"]), lambda: c.load_sos_f32(cs["butter5_padded"]),
              lambda: c.load_sos(cs["butter12"]), lambda: c.load_sos_f32(cs["rtl_default"])]
    return [states], lambda out: c.process_f32(x, out)


def _train_window(mode):
    def make(c, torch):
        """Float window: a table window, a cosine-fit window, the default.  Each setter uploads both window layouts and
        both plans' lane tables: four uploads, the whole staging ring, so the cycle runs as trains of two states."""
        c.load_sos(G2)
        c.set_filter_mode(mode)
        x = _x_f32(torch)
        states = [lambda: c.set_window_f32(_blackman()), lambda: c.set_window_f32(_hamming()),
                  lambda: c.set_window_f32(None)]
        return _pairs(states), lambda out: c.process_f32(x, out)
    return make


def _train_rom(mode):
    def make(c, torch):
        """Q15 window ROM: read by the FFT kernel in 0xB1 and by the cascade kernel in 0x00; one upload per state."""
        c.set_filter_mode(mode)
        x = _x_i16(torch)
        states = [lambda r=r: c.set_window_q15(r) for r in _roms()]
        return [states], lambda out: c.process_q15(x, out)
    return make


def _train_f64(c, torch):
    """Float64 tables: load_sos under set_precision('f64') uploads the lane table and both float64 plans (three
    uploads), so the cycle of three cascades runs as trains of two states."""
    cs = cascades()
    c.set_precision("f64")
    c.set_filter_mode(0xA1)
    x = _x_f32(torch)
    states = [lambda: c.load_sos(cs["long_memory"]), lambda: c.load_sos(cs["butter5_padded"]),
              lambda: c.load_sos(cs["butter12"])]
    return _pairs(states), lambda out: c.process_f32(x, out)


def _train_by_value(c, torch):
    """Settings passed by value with every launch (no upload): included for completeness.  Marker records of the integer
    chain depend on all five."""
    g4 = load_golden("g4_q15_frames.npz")                # (its first wide section has a zero numerator: left out)
    c12 = np.array([-14, 0, 14, 107, 21, 127, -15, 0, 15, 107, -21, 127], np.int8)      # imp/filter_pkg.vhd:54-68
    x = _x_i16(torch)

    def first():
        c.set_filter_mode(0xA1)
        c.load_coeffs_q7(g4["c_gui"])
        c.load_sos_q14(g4["sos_q14"][1:3])
        c.set_window_mode_q15(0)
        c.set_marker_range(0, N)

    states = [first, lambda: c.load_coeffs_q7(c12), lambda: c.set_window_mode_q15(1),
              lambda: c.set_marker_range(100, 9000), lambda: c.set_filter_mode(0xA2),
              lambda: c.load_sos_q14(g4["sos_q14"][1:5])]
    return [states], lambda out: c.process_q15(x, out, out_kind="marker")


TRAINS = {"lane_table": _train_lane, "window_f32_B1": _train_window(0xB1), "window_f32_A1": _train_window(0xA1),
          "rom_q15_B1": _train_rom(0xB1), "rom_q15_00": _train_rom(0x00), "tables_f64": _train_f64,
          "by_value": _train_by_value}


def _references(c, torch, states, call):
    """Each state's output with a synchronise after every call; they must differ pairwise, or a stale table could go
    unnoticed.  Leaves the handle in states[0], idle."""
    refs = []
    for st in states:
        st()
        o = call(None)
        torch.cuda.synchronize()
        refs.append(o.clone())
    for a, b in itertools.combinations(range(len(refs)), 2):
        assert not torch.equal(refs[a], refs[b]), f"states {a} and {b} give the same output: the train cannot tell them apart"
    states[0]()
    torch.cuda.synchronize()
    return refs


def _run_train(env, c, S, F, states, call, form, hold_ms, what):
    """states[0] is in place and the device idle.  [hold on S] call, setter, call, setter, call ... with no host
    synchronisation; then one synchronise.  The outputs, in call order."""
    torch = env.torch
    refs = _references(c, torch, states, call)
    depth = {"overlap2": 2, "overlap3": 3}.get(form, 1)
    with torch.cuda.stream(S):
        c.set_overlap(depth)
        if depth > 1:                       # the first overlapped call from S fits the internal streams: a host wait
            call(None)
            c.flush()
        outs = [torch.empty_like(refs[0]) for _ in states]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    end = env.hold(hold_ms, S) if hold_ms else None
    for j, st in enumerate(states):
        if j:
            st()
        with torch.cuda.stream(F if form == "alternating" and j % 2 else S):
            call(outs[j])
    if end is not None:
        _vacuity(env, end, t0, what, hold_ms)
    if depth > 1:
        with torch.cuda.stream(S):
            c.flush()
    torch.cuda.synchronize()
    bad = [j for j in range(len(states)) if not torch.equal(outs[j], refs[j])]
    stale = {j: [i for i in range(len(states)) if torch.equal(outs[j], refs[i])] for j in bad}
    assert not bad, f"{what}: calls {bad} of {len(states)} ran with another state's tables (output equals state: {stale})"


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("train", list(TRAINS))
def test_train_behind_a_hold(env, plane, train, form):
    """A hold on the caller's stream, then calls and setters with no host synchronisation: call j must run with state j,
    bit for bit what it gives with a synchronise after every call.  At most four uploads ride behind one hold (the
    staging ring has four slots; a fifth blocks the host until the hold ends).  Measured: the enqueues of a train took
    0.11 .. 0.74 ms of host time against H = 40 ms (FIGURE lines); the test asks for H >= 4 x that figure."""
    c, S, F = plane
    try:
        _reset(c)
        segments, call = TRAINS[train](c, env.torch)
        for n, states in enumerate(segments):
            _run_train(env, c, S, F, states, call, form, HOLD_MS, f"{train}/{form}/{n}")
    finally:
        env.torch.cuda.synchronize()
        _reset(c)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["ordered", "overlap2"])
def test_train_wraps_the_staging_ring(env, plane, form):
    """Twelve ROM uploads in one train with no hold: every staging slot is reused three times.  Results only."""
    c, S, F = plane
    try:
        _reset(c)
        x = _x_i16(env.torch)
        roms = _roms()
        states = [lambda r=r: c.set_window_q15(r) for r in roms]
        call = lambda out: c.process_q15(x, out)                       # noqa: E731
        torch = env.torch
        refs = _references(c, torch, states, call)
        order = [j % len(states) for j in range(13)]
        with torch.cuda.stream(S):
            c.set_overlap(2 if form == "overlap2" else 1)
            outs = [torch.empty_like(refs[0]) for _ in order]
            for n, j in enumerate(order):
                if n:
                    states[j]()
                call(outs[n])
            c.flush()
        torch.cuda.synchronize()
        bad = [n for n, j in enumerate(order) if not torch.equal(outs[n], refs[j])]
        assert not bad, f"calls {bad} ran with another state's ROM"
    finally:
        env.torch.cuda.synchronize()
        _reset(c)


# ------------------------------------------------------------------------------ part 5: join visibility in overlap mode
@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 3])
def test_joined_result_is_visible_on_the_callers_stream(env, plane, depth):
    """B = 2048 float frames in 0xA1.  Call k sits behind a hold on the caller's stream; once call k + d - 1 has been
    made, a clone of out[k][-1] enqueued on the caller's stream must hold the result (out was NaN before).  Not
    deterministic by construction: without the join the clone races with the kernel, and the margin is that the last
    frame of 2048 is written at the kernel's end.  Measured: the enqueues took 0.08 .. 0.10 ms against H = 40 ms."""
    c, S, F = plane
    torch = env.torch
    B = 2048
    try:
        _reset(c)
        c.load_sos(G2)
        c.set_filter_mode(0xA1)
        x = torch.from_numpy((0.3 * np.random.default_rng(51).standard_normal((B, N))).astype(np.float32)).cuda()
        with torch.cuda.stream(S):
            ref_last = c.process_f32(x)[-1].clone()
            torch.cuda.synchronize()
            c.set_overlap(depth)
            outs = [torch.empty((B, N), dtype=torch.float32, device="cuda") for _ in range(depth)]
            c.process_f32(x, outs[0])           # fits the internal streams to S (a host wait), and a first call k - 1
            c.flush()
            torch.cuda.synchronize()
            for o in outs:
                o.fill_(float("nan"))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            end = env.hold(HOLD_MS, S)
            for o in outs:                       # calls k .. k + d - 1
                c.process_f32(x, o)
            seen = outs[0][-1].clone()
            _vacuity(env, end, t0, f"join visibility depth {depth}")
            c.flush()
        torch.cuda.synchronize()
        assert torch.equal(outs[0][-1], ref_last)
        assert torch.equal(seen, ref_last), "the caller's stream read out[k] before call k's kernel had written it"
    finally:
        torch.cuda.synchronize()
        _reset(c)


# ------------------------------------------------------------------------------------------------------------ the sum
@pytest.mark.gpu
def test_zz_holds_add_up_to_seconds(env):
    print(f"FIGURE holds enqueued by this module: {env.held_ms / 1e3:.2f} s in all, each one wave and at most {HOLD_MS} ms")
    assert env.held_ms < 10000
