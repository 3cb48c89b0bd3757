"""GPU: the virtual board and the device's display outputs against fixture G7 -- the byte sessions the reference GUI's own
caller code writes and the numbers it shows, recorded by oracle/gui_sessions.py.  Every recorded open / write / buffer
reset / close is replayed on VirtualSerial objects over one VirtualFpga per session, with the board's state after each event
taken from the RTL table of gui_session_cases.Board, not from virtual_fpga.py.  Everything is exact; recorded gaps are not
slept."""
import hashlib
import socket
import threading

import numpy as np
import pytest

import gui_session_cases as gs
from gui_session_cases import CLOSE, FLUSH, FRAMES, OPEN, RESET_IN, RESET_OUT, UART, WRITE
from gpu_support import ch, to_device, torch_mod  # noqa: F401 (fixtures)
from udp_collect import FrameCollector

pytestmark = pytest.mark.gpu

G = gs.fixture()
SESSIONS = gs.session_names(G)
FRAME = 65536


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


class Replay:
    """One session on one virtual board (batch = 3), event by event."""

    def __init__(self, chain_cls, oracle, i):
        from fpga_real_time_fft_analyzer_amd.virtual_fpga import VirtualFpga, VirtualSerial
        self.oracle, self.i = oracle, i
        self.batches = []                      # the sample indices of every acquisition batch the board has asked for
        self.fpga = VirtualFpga(self._source, device=0, batch=3, chain=chain_cls(0))
        self.make = VirtualSerial.factory(self.fpga)
        self.board = gs.Board()
        self.ports = {}
        self.leftover = []                     # acquired under the control state in force, not yet on the wire
        self.wire = []                         # every frame read back, in order
        self._expected = {}

    def _source(self, n):
        k = sum(len(b) for b in self.batches)
        idx = [(k + j) % 3 for j in range(n)]
        self.batches.append(idx)
        return G["x"][idx]

    def open_port(self):
        live = [p for p in self.ports.values() if p.is_open]
        assert len(live) <= 1
        return live[0] if live else None

    def expected(self, idx):
        """The oracle's frame of sample ``idx`` under the control state the RTL table holds now."""
        key = (idx, self.board.mode, self.board.c12)
        if key not in self._expected:
            iq = self.oracle.chain_q15(G["x"][idx][None, :], None, 0, self.board.mode, self.board.coeffs, None)
            self._expected[key] = iq[0].astype("<i2").tobytes()
        return self._expected[key]

    def check_state(self, e):
        f, b = self.fpga, self.board
        got = (f.transport, f.started, f.uart_state, f.chain.filter_mode, f.chain.coeffs_q7().tobytes())
        assert got == b.state(), (SESSIONS[self.i], e)
        assert f.eth_streaming == b.eth_streaming
        if not b.eth_streaming:
            assert f.read_datagrams() == []
        port = self.open_port()
        if port is not None and b.uart != "STREAM":          # the UART is silent before 0xA5 (imp/sequ2.vhd:214-218)
            assert port.in_waiting == 0 and port.read(4096) == b""

    def apply(self, e):
        if e.kind == OPEN:
            assert self.open_port() is None
            self.ports[e.port] = self.make(*e.args, **e.kwargs)      # exactly the recorded arguments
            assert self.ports[e.port].is_open
        elif e.kind == WRITE:
            control = (self.board.mode, self.board.c12)
            assert self.ports[e.port].write(e.data) == len(e.data)
            self.board.write(e.data)
            if (self.board.mode, self.board.c12) != control or 0xFF in e.data:
                self.leftover = []                                   # frames computed ahead belong to the old settings
        elif e.kind == FLUSH:
            self.ports[e.port].flush()
        elif e.kind == RESET_IN:
            self.ports[e.port].reset_input_buffer()
        elif e.kind == RESET_OUT:
            self.ports[e.port].reset_output_buffer()
        elif e.kind == CLOSE:
            self.ports[e.port].close()                               # the board keeps its state: check_state follows
            assert not self.ports[e.port].is_open
            with pytest.raises(OSError):
                self.ports[e.port].write(b"\x55")
        elif e.kind == FRAMES:
            self.receive(e)
        self.check_state(e)

    def receive(self, e):
        fetched = len(self.batches)
        if e.via == UART:
            port, got = self.open_port(), bytearray()
            if e.n == 0:
                assert port.in_waiting == 0
            while len(got) < e.n * FRAME:                            # as read_data does, gui.py:623-627
                k = port.in_waiting
                assert k > 0
                got += port.read(min(k, 4096))
            out = [bytes(got[k * FRAME:(k + 1) * FRAME]) for k in range(e.n)]
            assert len(got) == e.n * FRAME
        else:
            dg = self.fpga.read_datagrams(e.n)
            assert len(dg) == 64 * e.n and all(len(d) == 1025 for d in dg)
            assert [d[0] for d in dg] == list(range(64)) * e.n
            asm = FrameCollector()
            out = [fr for fr in (asm.add(d, 0) for d in dg) if fr is not None]
        # the frames on the wire are the acquisitions made under the control state in force, in order, none skipped
        new = [i for b in self.batches[fetched:] for i in b]
        assert len(self.batches) - fetched == -(-max(0, e.n - len(self.leftover)) // 3)
        pool = self.leftover + new
        assert len(out) == e.n and out == [self.expected(i) for i in pool[:e.n]]
        self.leftover = pool[e.n:]
        self.wire += out

    def run(self, until_frames=False):
        for e in gs.events(G, self.i):
            if until_frames and e.kind == FRAMES:
                return
            self.apply(e)

    def close(self):
        self.fpga.close()


@pytest.mark.parametrize("i", range(len(SESSIONS)), ids=SESSIONS)
def test_session_replay(chain_cls, torch_mod, oracle, i):
    """Every recorded session: the board's transport, started flag, UART state, filter mode and coefficients after each
    event as imp/sequ2.vhd and new/command_control.vhd give them; a port the GUI closes leaves the board alone and the next
    port sees its state; the frames read back the way the GUI reads them are the oracle's, and hash to what the reference's
    receiver was handed."""
    r = Replay(chain_cls, oracle, i)
    try:
        assert r.fpga.transport == "ETHERNET" and not r.fpga.started          # imp/sequ2.vhd:85-86
        r.run()
        assert [sha(f) for f in r.wire] == [str(s) for s in G[f"s{i}_frame_sha"]]
    finally:
        r.close()


def test_ethernet_session_through_serve_udp(chain_cls, torch_mod, oracle):
    """The Ethernet start-up session up to its first frame, then two frames through serve_udp on a loopback socket."""
    i = SESSIONS.index("ethernet_startup")
    r = Replay(chain_cls, oracle, i)
    rx = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    try:
        r.run(until_frames=True)
        assert r.fpga.eth_streaming
        rx.setsockopt(socket.SOL_SOCKET, socket.SO_RCVBUF, 1 << 20)      # room for both frames' datagrams at once
        rx.bind(("127.0.0.1", 0))
        rx.settimeout(5.0)
        sent = []
        th = threading.Thread(target=lambda: sent.append(r.fpga.serve_udp(addr=rx.getsockname(), n_frames=2, fps_limit=200.0)))
        th.start()
        asm, got = FrameCollector(), []
        while len(got) < 2:
            p = rx.recv(2048)
            assert len(p) == 1025
            fr = asm.add(p, 0)
            if fr is not None:
                got.append(fr)
        th.join(timeout=10)
        assert sent == [2] and got == [r.expected(0), r.expected(1)]
        assert [sha(f) for f in got] == [str(s) for s in G[f"s{i}_frame_sha"][:2]]
    finally:
        rx.close()
        r.close()


SWEEPS = gs.sweeps(G)


@pytest.mark.parametrize("j", range(len(SWEEPS)), ids=[f"{SESSIONS[s[1]]}-{s[3]:02x}" for s in SWEEPS])
def test_device_outputs_meet_the_recorded_numbers(ch, torch_mod, j):
    """The device's own display outputs against what the GUI computed from the same frames: after the session's bytes
    through the command decoder, 'mag' hashes to the recorded SHA-256 row by row and range by range, 'iq' holds the recorded
    real / imaginary lists, and with set_marker_range(recorded bounds) the marker record has the bits of the recorded
    peak_magnitude and the recorded lower bound + peak_bin -- from int16 samples and, for the first and the filtered UART
    session, from the same samples packed to 12 bits."""
    from fpga_real_time_fft_analyzer_amd import ingest
    _, i, via, cmd, c12, n = SWEEPS[j]
    ch.feed_command_bytes(gs.written(G, i))
    assert ch.filter_mode == cmd and np.array_equal(ch.coeffs_q7(), c12)
    x = G["x"][:n]
    forms = [to_device(torch_mod, x)]
    if SESSIONS[i] in ("uart_startup", "filters_uart"):
        forms.append(to_device(torch_mod, ingest.pack12(x)))
    for xd in forms:
        mag = ch.process_q15(xd, out_kind="mag").cpu().numpy()
        iq = ch.process_q15(xd).cpu().numpy()
        assert mag.shape == (n, 16384) and mag.dtype == np.float32
        for r in range(8):
            lo, hi = G[f"w{j}_bounds"][r].tolist()
            for f in range(n):
                assert sha(np.ascontiguousarray(mag[f, lo:hi]).tobytes()) == str(G[f"w{j}_sha"][r, f]), (r, f)
            for key, part in (("re", 0), ("im", 1)):
                if f"w{j}_{key}_{r}" in G.files:
                    assert np.array_equal(iq[:, lo:hi, part], G[f"w{j}_{key}_{r}"])
            ch.set_marker_range(lo, hi)
            peak_mag, peak_bin, _ = ch.markers_q15(xd)
            bits = np.ascontiguousarray(peak_mag.cpu().numpy()).view(np.uint32)
            assert np.array_equal(bits, G[f"w{j}_peak_mag"][r].view(np.uint32)), r
            assert np.array_equal(peak_bin.cpu().numpy(), lo + G[f"w{j}_peak_bin"][r]), r
