"""Shared by test_gui_sessions_cpu.py and test_gpu_gui_sessions.py (a plain module, like structured_cases.py): fixture G7 --
the byte sessions and numbers recorded from the reference GUI's own caller code by oracle/gui_sessions.py -- read back as
events, and the board's state after each written byte as the RTL gives it."""
import json
import re
from collections import namedtuple

import numpy as np

from conftest import ROOT, load_golden

OPEN, WRITE, GAP, RESET_IN, RESET_OUT, CLOSE, FLUSH, FRAMES, TIMER, PAUSE = range(10)
UART, ETHERNET = 0, 1

# kind, port (order of construction in the session, -1: none), step name, data (bytes of a write), ms (gap / timer delay),
# args / kwargs (of an open), n / via (of FRAMES: how many frames the receiver was handed, UART or ETHERNET)
Event = namedtuple("Event", "kind port step data ms args kwargs n via")


def fixture():
    return load_golden("g7_gui_sessions.npz")


def session_names(g=None):
    return [str(s) for s in (fixture() if g is None else g)["session_names"]]


def events(g, i):
    """The events of session ``i`` in order."""
    ev, ms, blob = g[f"s{i}_ev"], g[f"s{i}_ms"], g[f"s{i}_bytes"].tobytes()
    steps, opens = g[f"s{i}_steps"], g[f"s{i}_opens"]
    out = []
    for (kind, port, step, a, b), gap in zip(ev.tolist(), ms.tolist()):
        o = json.loads(str(opens[a])) if kind == OPEN else {"args": None, "kwargs": None}
        out.append(Event(kind, port, str(steps[step]), blob[a:a + b] if kind == WRITE else b"", gap, o["args"], o["kwargs"],
                         a if kind == FRAMES else 0, b if kind == FRAMES else -1))
    return out


def written(g, i) -> bytes:
    return b"".join(e.data for e in events(g, i) if e.kind == WRITE)


def header_bytes() -> dict:
    """name -> value of every command and filter-mode byte include/specan.h defines."""
    txt = open(f"{ROOT}/include/specan.h").read()
    return {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define\s+(SA_(?:CMD|FILTER)_\w+)\s+0x([0-9A-Fa-f]{2})\b", txt)}


def cut_commands(stream: bytes):
    """A write stream cut by the command decoder's rules: ``(command byte, data)`` with 12 data bytes after 0xF1
    (new/rx_filter_coeff.vhd:45-56) and none after anything else.  A stream that ends inside an upload gives a short data."""
    out, i = [], 0
    while i < len(stream):
        k = 13 if stream[i] == 0xF1 else 1
        out.append((stream[i], stream[i + 1:i + k]))
        i += k
    return out


class Board:
    """What the RTL holds after each byte the host writes.  Power-on and reset state: Ethernet selected
    (imp/sequ2.vhd:85-86), both output machines idle (:101-102, :182-183), filter mode 0xB1 (new/command_control.vhd:31, :50),
    custom coefficients zero (new/filter_iir12_cust.vhd:51-52).  ``uart`` is IDLE1 / IDLE2 / STREAM as in virtual_fpga.py:
    U_IDLE1, U_IDLE2, and everything from U_READ on."""

    def __init__(self):
        self._upload = None                 # the coefficient bytes taken so far while new/rx_filter_coeff.vhd is busy
        self._reset()

    def _reset(self):                       # 0xFF: command_control.vhd:59-60 pulls the reset every block above takes
        self.transport, self.eth_streaming, self.uart = "ETHERNET", False, "IDLE1"
        self.mode, self.c12 = 0xB1, bytes(12)

    def _mode(self, b):                     # command_control.vhd:53-58
        self.mode = b

    def _ethernet(self, b):                 # sequ2.vhd:88-89; the UART machine idles while Ethernet is selected (:253-254)
        self.transport, self.uart = "ETHERNET", "IDLE1"

    def _uart(self, b):                     # sequ2.vhd:90-91; the Ethernet machine idles while the UART is selected (:173-174)
        self.transport, self.eth_streaming = "UART", False

    def _start(self, b):                    # command_control.vhd:61-62 -> start_fill, seen by the selected machine only
        if self.transport == "ETHERNET":
            self.eth_streaming = True       # S_IDLE1 -> S_FILL, sequ2.vhd:122-127
        elif self.uart == "IDLE1":
            self.uart = "IDLE2"             # U_IDLE1 -> U_IDLE2, sequ2.vhd:205-209

    def _request(self, b):                  # U_IDLE2 -> U_READ on 0xA5, sequ2.vhd:214-218; ignored everywhere else
        if self.transport == "UART" and self.uart == "IDLE2":
            self.uart = "STREAM"

    def _begin_upload(self, b):             # new/rx_filter_coeff.vhd:45-56: the next 12 bytes are data for nobody else
        self._upload = bytearray()

    COMMANDS = {0x00: _mode, 0xA1: _mode, 0xB1: _mode, 0xFF: lambda self, b: self._reset(), 0xEF: _ethernet, 0xFE: _uart,
                0x55: _start, 0xA5: _request, 0xF1: _begin_upload}

    def write(self, data: bytes):
        for b in bytes(data):
            if self._upload is not None:    # busy: neither decoder sees the byte (imp/dsp_system_top.vhd:644)
                self._upload.append(b)
                if len(self._upload) == 12:
                    self.c12, self._upload = bytes(self._upload), None
            elif b in self.COMMANDS:
                self.COMMANDS[b](self, b)   # any other byte: no effect

    @property
    def started(self) -> bool:
        return self.eth_streaming or self.uart != "IDLE1"

    @property
    def coeffs(self) -> np.ndarray:
        return np.frombuffer(self.c12, np.int8)

    def state(self) -> tuple:
        return self.transport, self.started, self.uart, self.mode, self.c12


def final_board(g, i) -> Board:
    b = Board()
    b.write(written(g, i))
    return b


def sweeps(g):
    """(j, session, transport, filter command, 12 coefficients, frames per range) of each recorded sweep."""
    return [(j, int(g["sweep_session"][j]), int(g["sweep_transport"][j]), int(g["sweep_cmd"][j]), g["sweep_c12"][j],
             int(g["sweep_frames"][j])) for j in range(len(g["sweep_session"]))]


def oracle_frames(oracle, g, n, cmd, c12):
    """Frames 0..n-1 of the fixture's samples under (cmd, c12): [n, 16384, 2] int16."""
    return oracle.chain_q15(g["x"][:n], None, 0, cmd, np.asarray(c12, np.int8), None)
