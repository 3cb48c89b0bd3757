"""CPU: fixture G7 -- the byte sessions and display numbers recorded from the reference GUI's own caller code
(oracle/gui_sessions.py lists the arrays) -- against the package's host helpers: the coefficient upload bytes, the per-mille
range, the frame decoder, the marker mirror and the UDP cut.  Everything is exact."""
import hashlib
import json
import os
import types

import numpy as np
import pytest

from conftest import GOLDEN, N, load_golden
from oracle import gui_sessions as recorder
from udp_collect import FrameCollector
import gui_session_cases as gs
from gui_session_cases import CLOSE, ETHERNET, FLUSH, FRAMES, GAP, OPEN, TIMER, UART, WRITE

SESSIONS = ["uart_startup", "ethernet_startup", "mode_switch", "mode_switch_busy_main_thread", "filters_uart",
            "filters_ethernet", "reset_cooldown"]
TEMP_PORT = {"timeout": 1.0}                                       # gui.py:780, 886, 939, 1022, 1252
RECEIVER_PORT = {"timeout": 0.001, "writeTimeout": 0.5, "rtscts": False, "dsrdtr": False, "xonxoff": False,
                 "exclusive": True}                                # gui.py:469-478


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


@pytest.fixture(scope="module")
def g():
    return gs.fixture()


@pytest.fixture(scope="module")
def swept_frames(g, oracle):
    """sweep -> the oracle's frames for the fixture's samples under the sweep's filter state, as bytes; computed once."""
    return {j: [f.astype("<i2").tobytes() for f in gs.oracle_frames(oracle, g, n, cmd, c12)]
            for j, _, _, cmd, c12, n in gs.sweeps(g)}


# ---------------------------------------------------------------------------------------------- the fixture itself
def test_fixture_holds_arrays_only(g):
    assert os.path.getsize(os.path.join(GOLDEN, "g7_gui_sessions.npz")) < 512 * 1024
    assert gs.session_names(g) == SESSIONS
    for name in g.files:                                           # load_golden refuses pickles; these are plain arrays
        assert g[name].dtype.kind in "iufU", name
    assert g["x"].shape == (3, N) and g["x"].dtype == np.int16 and np.abs(g["x"].astype(int) + 0.5).max() <= 2047.5
    assert g["ranges"].tolist() == [[0, 1000], [0, 500], [250, 500], [123.4, 567.8], [999.95, 1000], [500, 500],
                                    [1000, 1000], [700, 300]]
    assert sorted(int(g["sweep_cmd"][j]) for j in range(len(g["sweep_cmd"]))) == [0x00, 0xA1, 0xA1, 0xA1, 0xB1]
    assert g["sweep_frames"].max() <= 3


@pytest.mark.parametrize("i", range(len(SESSIONS)), ids=SESSIONS)
def test_ports_and_write_streams_are_well_formed(g, i):
    """Ports are numbered as they are opened, used only while open, one at a time (the receiver's is exclusive); the write
    stream, cut as the command decoder cuts it, holds nothing but bytes include/specan.h defines; no session hands the
    receiver more than 3 frames at once."""
    defined = gs.header_bytes()
    gui_bytes = set(load_golden("g6_frame.npz")["cmds"].tolist())      # gui.py:28-37
    assert gui_bytes == set(defined.values()) - {defined["SA_FILTER_WIDE"]}
    open_port, n_ports, per_port = None, 0, {}
    for e in gs.events(g, i):
        if e.kind == OPEN:
            assert open_port is None and e.port == n_ports
            assert e.args == ["COM5", 230400] and e.kwargs in (TEMP_PORT, RECEIVER_PORT)      # gui.py:23-24
            open_port, n_ports = e.port, n_ports + 1
        elif e.kind in (WRITE, FLUSH, CLOSE, gs.RESET_IN, gs.RESET_OUT):
            assert e.port == open_port, e
            if e.kind == WRITE:
                per_port.setdefault(e.port, bytearray()).extend(e.data)
            if e.kind == CLOSE:
                open_port = None
        else:
            assert e.port == -1 and (e.kind != FRAMES or 0 <= e.n <= 3)
    cut = gs.cut_commands(gs.written(g, i))
    assert cut and all(cmd in gui_bytes and len(data) == (12 if cmd == 0xF1 else 0) for cmd, data in cut)
    for stream in per_port.values():                                   # no upload straddles two ports
        assert all(len(data) == (12 if cmd == 0xF1 else 0) for cmd, data in gs.cut_commands(bytes(stream)))


def test_sessions_take_the_paths_they_are_named_for(g):
    ev = {name: gs.events(g, i) for i, name in enumerate(SESSIONS)}
    kw = {name: {e.port: e.kwargs for e in ev[name] if e.kind == OPEN} for name in SESSIONS}

    def writes(name, byte):
        return [e for e in ev[name] if e.kind == WRITE and e.data == bytes([byte])]

    # start-up: the mode byte through a temporary port, then (UART) the receiver's port with both buffers reset
    for name in SESSIONS:
        first = [e for e in ev[name] if e.kind in (OPEN, WRITE, CLOSE)][:3]
        mode = 0xEF if "ethernet" in name else 0xFE
        assert [e.kind for e in first] == [OPEN, WRITE, CLOSE] and first[0].kwargs == TEMP_PORT and first[1].data == bytes([mode])
    kinds = [e.kind for e in ev["uart_startup"]]
    assert kinds[kinds.index(CLOSE) + 1:][:3] == [OPEN, gs.RESET_IN, gs.RESET_OUT]
    # 0x55, a 100 ms single-shot timer, 0xA5 -- on the receiver's port
    for name in ("uart_startup", "mode_switch", "filters_uart", "reset_cooldown"):
        seq = [e for e in ev[name] if e.kind in (WRITE, TIMER)]
        k = next(k for k, e in enumerate(seq) if e.data == b"\x55")
        assert seq[k + 1].kind == TIMER and seq[k + 1].ms == 100.0 and seq[k + 2].data == b"\xA5"
        assert kw[name][seq[k].port] == RECEIVER_PORT and seq[k + 2].port == seq[k].port
    # Ethernet: every command through a port of its own that is closed again
    for name in ("ethernet_startup", "filters_ethernet"):
        assert all(k == TEMP_PORT for k in kw[name].values())
        assert not writes(name, 0xA5) and len(writes(name, 0x55)) == 1
    # a mode switch: three 0xFF, 100 ms after each, through a temporary port -- or on the receiver's port when the Qt thread
    # has not stopped the receiver yet (force_mode_reset); then the mode byte through a temporary port
    for name, want in (("mode_switch", [TEMP_PORT, TEMP_PORT]), ("mode_switch_busy_main_thread", [RECEIVER_PORT, TEMP_PORT])):
        resets = writes(name, 0xFF)
        assert len(resets) == 6 and [kw[name][e.port] for e in resets[::3]] == want
        seq = [e for e in ev[name] if e.kind in (WRITE, GAP)]
        for e in resets:
            nxt = seq[seq.index(e) + 1]
            assert nxt.kind == GAP and nxt.ms == 100.0
        assert [kw[name][e.port] for e in writes(name, 0xEF) + writes(name, 0xFE)[1:]] == [TEMP_PORT, TEMP_PORT]
    # resets: three asked for, the one inside the 2 s cool-down never reaches the port
    steps = [str(s) for s in g[f"s{SESSIONS.index('reset_cooldown')}_steps"]]
    assert steps.count("handle_fpga_reset") == 3 and len(writes("reset_cooldown", 0xFF)) == 2
    asked = [k for k, s in enumerate(steps) if s == "handle_fpga_reset"]
    assert steps[asked[0] + 1] == "pause 0.5 s" and steps[asked[1] + 1] == "pause 2 s"
    wrote = [sum(e.kind == WRITE for e in ev["reset_cooldown"][a:b]) for a, b in _step_spans(g, "reset_cooldown", asked)]
    assert wrote == [1, 0, 1]


def _step_spans(g, name, step_indices):
    """[first, last + 1) event rows of the given steps of a session."""
    rows = g[f"s{SESSIONS.index(name)}_ev"][:, 2]
    return [(int(np.searchsorted(rows, k, "left")), int(np.searchsorted(rows, k, "right"))) for k in step_indices]


def test_board_model_at_the_receiver(g, oracle):
    """What the recorder handed the receiver is what the RTL would stream then: frames under the filter state the written
    bytes leave, on the selected transport, after 0x55 (and 0xA5 on the UART) -- and nothing where the RTL is silent: the
    reset of the last session leaves the board on Ethernet (imp/sequ2.vhd:85-86) while the GUI listens on the UART."""
    for i, name in enumerate(SESSIONS):
        board, k = gs.Board(), 0
        shas = [str(s) for s in g[f"s{i}_frame_sha"]]
        for e in gs.events(g, i):
            board.write(e.data)
            if e.kind != FRAMES:
                continue
            streaming = board.uart == "STREAM" if e.via == UART else board.eth_streaming
            assert (e.n > 0) == streaming, (name, e)
            want = gs.oracle_frames(oracle, g, e.n, board.mode, board.coeffs) if e.n else []
            assert shas[k:k + e.n] == [sha(f.astype("<i2").tobytes()) for f in want]
            k += e.n
        assert k == len(shas) == len(g[f"s{i}_counters"])
    assert gs.final_board(g, SESSIONS.index("reset_cooldown")).transport == "ETHERNET"


def test_sweeps_run_under_the_state_their_session_ends_in(g):
    for j, i, via, cmd, c12, n in gs.sweeps(g):
        board = gs.final_board(g, i)
        assert (board.mode, board.c12) == (cmd, c12.tobytes()), SESSIONS[i]
    assert not g["sweep_c12"][-1].any() and g["sweep_cmd"][-1] == 0xA1      # custom selected after a reset, nothing uploaded


# ---------------------------------------------------------------------------------------------- coefficient uploads
def _designs_and_uploads(g, i):
    """(design given to update_filter_config, the 12 bytes uploaded for it) in order."""
    steps = [str(s) for s in g[f"s{i}_steps"]]
    designs, last = [], None
    for s in steps:
        if s.startswith("handle_update_filter_config "):
            last = json.loads(s.split(" ", 1)[1])
        elif s == "handle_apply_filter_to_fpga":
            designs.append(last)
    uploads = [data for cmd, data in gs.cut_commands(gs.written(g, i)) if cmd == 0xF1]
    assert len(designs) == len(uploads)
    return list(zip(designs, uploads))


@pytest.mark.parametrize("name", ["filters_uart", "filters_ethernet", "reset_cooldown"])
def test_package_helpers_produce_the_recorded_upload_bytes(g, name):
    """designer.design_iir_filter -> quantize_coefficients -> two_sections_for_fpga -> coefficient_upload_bytes, and the byte
    assembly of SpectrumChain.send_filter_coefficients, give the bytes the GUI wrote: through UartReceiver
    (``int(c) & 0xFF``, gui.py:603) and through the temporary port (``tobytes()[0]`` of the numpy integers, gui.py:791-794)."""
    from fpga_real_time_fft_analyzer_amd import designer
    from fpga_real_time_fft_analyzer_amd.chain import SpectrumChain
    pairs = _designs_and_uploads(g, SESSIONS.index(name))
    assert len(pairs) == (1 if name == "reset_cooldown" else 4)
    n_sections = []
    for d, recorded in pairs:
        sos = designer.design_iir_filter(d["filter_type"], d["filter_order"], d["cutoff_freq"], d["cutoff_freq2"], d["sample_rate"])
        q = designer.quantize_coefficients(sos)
        n_sections.append(len(q))
        assert all(isinstance(c, np.int8) for s in q for c in s)
        two = designer.two_sections_for_fpga(q)
        assert len(two) == 2 and bytes(c & 0xFF for s in two for c in s) == recorded
        assert designer.coefficient_upload_bytes(q) == b"\xF1" + recorded
        if len(q) < 2:                                             # padded with the pass-through section, gui.py:1190
            assert recorded[6:] == bytes([64, 0, 0, 64, 0, 0])
        # the numpy-integer path: the sections as the GUI holds them -- numpy int8 where designed, Python ints where padded
        as_gui = [list(s) for s in q[:2]] + [[64, 0, 0, 64, 0, 0]] * (2 - len(q[:2]))
        for sections in (two, as_gui):
            fed = []
            stub = types.SimpleNamespace(feed_command_bytes=fed.append)
            assert SpectrumChain.send_filter_coefficients(stub, sections) == b"\xF1" + recorded == fed[0] and len(fed) == 1
        assert bytes(np.asarray(as_gui, np.int8).reshape(12).view(np.uint8)) == recorded
    if name != "reset_cooldown":                                   # one section (padded), three (cut), two: all there
        assert sorted(n_sections) == [1, 2, 2, 3]


# ---------------------------------------------------------------------------------------------- range, decoder, markers
def test_bin_range_from_permille_gives_the_recorded_slice_bounds(g):
    from fpga_real_time_fft_analyzer_amd.frames import bin_range_from_permille
    want = [(0, N), (0, 8192), (4096, 8192), (2021, 9302), (16383, N), (8192, 8193), (16383, N), (11468, 11469)]
    for j, *_ in gs.sweeps(g):
        for r, (start, end) in enumerate(g["ranges"].tolist()):
            lo, hi = bin_range_from_permille(start, end)
            assert [lo, hi] == g[f"w{j}_bounds"][r].tolist() == list(want[r])     # the recorded bounds, by hand as well
            assert (g[f"w{j}_len"][r] == hi - lo).all()


def test_decoder_slice_and_marker_give_the_recorded_numbers(g, swept_frames):
    """Per sweep, range and frame: the hash of the sliced magnitudes, peak_magnitude (float32 bits) and peak_bin of the
    GUI's frame_data payload, its real / imaginary lists and its frame counters -- from frames.decode_mag_16iq_le,
    decode_iq_components, max / argmax and frames.marker_of_frame on the oracle's frame."""
    from fpga_real_time_fft_analyzer_amd import frames
    for j, i, via, cmd, c12, n in gs.sweeps(g):
        before = len(g[f"s{i}_counters"])                          # the counters run on from the session's own frames
        for f in range(n):
            frame = swept_frames[j][f]
            mag = frames.decode_mag_16iq_le(frame)
            re, im = frames.decode_iq_components(frame)
            assert mag.dtype == np.float32
            for r in range(8):
                lo, hi = g[f"w{j}_bounds"][r].tolist()
                assert sha(frame) == str(g[f"w{j}_frame_sha"][r, f])
                assert sha(mag[lo:hi].tobytes()) == str(g[f"w{j}_sha"][r, f]), (j, r, f)
                peak, rel = g[f"w{j}_peak_mag"][r, f], int(g[f"w{j}_peak_bin"][r, f])
                assert mag[lo:hi].max().view(np.uint32) == peak.view(np.uint32) and int(mag[lo:hi].argmax()) == rel
                pm, pb, _ = frames.marker_of_frame(frame, lo, hi)
                assert pm.view(np.uint32) == peak.view(np.uint32) and pb == lo + rel
                plots = str(g["range_plots"][r]).split(",")
                for key, a in (("re", re), ("im", im)):
                    name = f"w{j}_{key}_{r}"
                    assert (name in g.files) == ({"re": "real", "im": "imaginary"}[key] in plots)
                    if name in g.files:
                        assert np.array_equal(g[name][f].astype(np.float32), a[lo:hi])
                assert g[f"w{j}_received"][r, f] == g[f"w{j}_displayed"][r, f] == before + r * n + f + 1
    # the filtered frames are small numbers with many equal magnitudes: the first of them is the peak (np.argmax)
    assert any((g[f"w{j}_peak_mag"] <= 5).all() for j, *_ in gs.sweeps(g))


def test_udp_cut_reassembles_to_the_frames_the_reference_assembled(g, swept_frames):
    """frames.frame_to_udp_payloads then FrameCollector: the frames MultiPacketAssembler handed the decoder (their recorded
    hashes), for every frame that reached the GUI as datagrams."""
    from fpga_real_time_fft_analyzer_amd import frames
    checked = 0
    for j, i, via, cmd, c12, n in gs.sweeps(g):
        if via != ETHERNET:
            continue
        for f in range(n):
            payloads = frames.frame_to_udp_payloads(swept_frames[j][f])
            assert len(payloads) == 64 and all(len(p) == 1025 and p[0] == k for k, p in enumerate(payloads))
            asm = FrameCollector()
            out = [fr for fr in (asm.add(p, 0) for p in payloads) if fr is not None]
            assert len(out) == 1 and sha(out[0]) == str(g[f"w{j}_frame_sha"][0, f])
            checked += 1
    assert checked == 5


# ---------------------------------------------------------------------------------------------- regeneration
@pytest.mark.skipif(not os.path.exists(recorder.GUI_PATH),
                    reason="the reference GUI is not on this machine: the sessions cannot be recorded again")
def test_regenerated_sessions_equal_the_committed_fixture(g, oracle):
    fresh = recorder.record_all()
    assert sorted(fresh) == sorted(g.files)
    for name in g.files:
        a, b = np.asarray(fresh[name]), g[name]
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), name
