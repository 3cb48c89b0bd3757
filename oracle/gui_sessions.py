"""Record what the reference GUI writes and computes: tests/golden/g7_gui_sessions.npz.
RUNS ONLY WHERE THE REFERENCE IS PRESENT (gen_golden.REF); called by gen_golden.main().

The reference's own caller code (scripts/fft_analyzer_gui.py: the socket handlers, ReceiverController, UartReceiver,
UdpReceiver and the start-up block under ``__main__``) is imported and run here against stand-ins written for this build:

  * Qt: ``QObject``, a ``pyqtSignal`` with connect / emit, ``pyqtSlot``, a ``QTimer`` with a ``timeout`` signal, start / stop
    and a ``singleShot`` that logs its delay and runs the callable at once, ``QMetaObject.invokeMethod`` + ``Q_ARG`` that call
    the named method directly (or, for the "busy main thread" session, queue the call until the handler has returned -- the
    order a queued connection gives when the Qt thread is slower than the handler's sleeps), ``QTime``, ``QUdpSocket``;
  * ``flask_socketio``: a ``SocketIO`` whose ``on`` leaves the handlers callable and whose ``emit`` keeps every payload;
  * ``serial``: a ``Serial`` that logs its constructor arguments and every write / flush / buffer reset / close, and serves
    ``in_waiting`` / ``read`` from a byte buffer the recorder fills;
  * the name ``time`` inside the imported module: a clock whose ``sleep`` advances it and logs the gap.  Nothing sleeps and
    the global ``time`` module is left alone.

Only data is stored -- byte strings, numbers, names of steps -- never text of the reference or anything compiled from it.

Arrays of g7_gui_sessions.npz
  x                 int16 [3,16384]   12-bit tone + noise samples every session and sweep is served from
  ranges            float64 [8,2]     the per-mille ranges of the sweeps, as given to handle_apply_frequency_range
  range_plots       str [8]           the plot types switched on with each range, comma separated
  session_names     str [S]
  per session i (events in order, one row each):
  s{i}_steps        str [..]          names of the steps (entry points called); events carry an index into it
  s{i}_ev           int32 [E,5]       (kind, port, step, a, b).  kind: 0 open (a: row of s{i}_opens), 1 write (a, b: offset and
                                      length in s{i}_bytes), 2 gap slept by the reference, 3 reset_input_buffer,
                                      4 reset_output_buffer, 5 close, 6 flush, 7 frames handed to the receiver (a: how many,
                                      b: 0 UART read_data / 1 UDP process_payload), 8 single-shot timer, 9 gap made by the recorder
                                      (the clock moved between two user actions).  port numbers the Serial objects of the
                                      session in order of construction, -1 where none is meant
  s{i}_ms           float64 [E]       the gap or timer delay in ms of kinds 2, 8, 9; 0 elsewhere
  s{i}_bytes        uint8 [..]        every written byte of the session, in order
  s{i}_opens        str [..]          JSON {"args": [...], "kwargs": {...}} of each Serial(...)
  s{i}_counters     int32 [F,2]       frames_received, frames_displayed in each frame_data payload of the session's kind-7 events
  s{i}_frame_sha    str [F]           SHA-256 of each frame the receiver cut / assembled there
  sweep_session     int32 [W]         the session each sweep closes
  sweep_transport   int32 [W]         0 UartReceiver.read_data in chunks of at most 4096 bytes, 1 UdpReceiver.process_payload
  sweep_cmd         uint8 [W]         the filter mode the session ends in
  sweep_c12         int8 [W,12]       the coefficient bytes the board holds then
  sweep_frames      int32 [W]         frames per range (at most 3; frame f is made of x[f])
  per sweep j, from the frame_data payloads ([8 ranges, n frames] unless noted):
  w{j}_peak_mag     float32           peak_magnitude
  w{j}_peak_bin     int32             peak_bin (within the slice)
  w{j}_len          int32             length of the frequency list == of the magnitude list
  w{j}_bounds       int32 [8,2]       first and last + 1 of an index ramp passed through get_frequency_range_data
  w{j}_sha          str               SHA-256 of the magnitude list as float32 bytes
  w{j}_received, w{j}_displayed  int32   the counters in the payload
  w{j}_frame_sha    str               SHA-256 of the frame the receiver cut / assembled
  w{j}_re_{r}, w{j}_im_{r}  int16 [n, len]   the sliced 'real' / 'imaginary' lists of range r where that plot type is on
                                      (whole numbers; the recorder checks that int16 holds them exactly)
"""
from __future__ import annotations

import ast
import contextlib
import hashlib
import importlib.util
import io
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = "/root/reference"
GUI_PATH = os.path.join(REF, "scripts", "fft_analyzer_gui.py")
FIXTURE = os.path.join(ROOT, "tests", "golden", "g7_gui_sessions.npz")
N = 16384

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OPEN, WRITE, GAP, RESET_IN, RESET_OUT, CLOSE, FLUSH, FRAMES, TIMER, PAUSE = range(10)

RANGES = [(0, 1000), (0, 500), (250, 500), (123.4, 567.8), (999.95, 1000), (500, 500), (1000, 1000), (700, 300)]
RANGE_PLOTS = ["magnitude", "magnitude", "magnitude,real", "magnitude,imaginary", "magnitude,real,imaginary",
               "magnitude,real,imaginary", "magnitude,real,imaginary", "magnitude,real,imaginary"]


def sha(b) -> str:
    return hashlib.sha256(bytes(b)).hexdigest()


# ------------------------------------------------------------------------------------------------ the log
class Log:
    """The events of one session, in order."""

    def __init__(self):
        self.events: list = []          # (kind, port, step, payload)
        self.steps: list = []
        self.ports = 0
        self.emitted: list = []         # (event name, payload) of every socketio.emit / emit
        self.frames: list = []          # every frame the receiver handed to its decoder
        self.t = 1000.0                 # the module's clock, seconds

    def step(self, name: str):
        self.steps.append(name)

    def add(self, kind: int, port: int = -1, payload=None):
        self.events.append((kind, port, len(self.steps) - 1, payload))

    def written(self) -> bytes:
        return b"".join(p for k, _, _, p in self.events if k == WRITE)


class Clock:
    """Stands for the name ``time`` in the imported module."""

    def __init__(self, log: Log):
        self._log = log

    def time(self) -> float:
        return self._log.t

    def sleep(self, seconds: float):
        self._log.t += float(seconds)
        self._log.add(GAP, -1, float(seconds) * 1e3)


# ------------------------------------------------------------------------------------------------ stand-ins
class _BoundSignal:
    def __init__(self):
        self._slots = []

    def connect(self, slot):
        self._slots.append(slot)

    def emit(self, *args):
        for s in list(self._slots):
            s(*args)


class _Signal:
    """pyqtSignal: a class attribute that gives every instance a signal of its own."""

    def __init__(self, *types_, **kw):
        self._name = None

    def __set_name__(self, owner, name):
        self._name = "_sig_" + name

    def __get__(self, obj, owner=None):
        if obj is None:
            return self
        return obj.__dict__.setdefault(self._name, _BoundSignal())


class _QObject:
    def __init__(self, *a, **k):
        pass

    def deleteLater(self):
        pass


def _make_modules(log: Log, queued: list | None):
    """Fresh PyQt5 / flask_socketio / serial stand-ins bound to ``log``.  With ``queued`` a list, invokeMethod appends the
    call to it instead of making it."""
    qtcore = types.ModuleType("PyQt5.QtCore")

    class QTimer(_QObject):
        def __init__(self, *a, **k):
            self.timeout = _BoundSignal()
            self.interval = None

        def start(self, ms=0):
            self.interval = ms

        def stop(self):
            self.interval = None

        @staticmethod
        def singleShot(ms, fn):
            log.add(TIMER, -1, float(ms))
            log.t += ms / 1e3
            fn()

    class QTime:
        @staticmethod
        def currentTime():
            return QTime()

        def msecsSinceStartOfDay(self):
            return int((log.t % 86400.0) * 1e3)

    class QMetaObject:
        @staticmethod
        def invokeMethod(obj, name, *rest):
            args = tuple(a.value for a in rest if isinstance(a, _Arg))
            if queued is not None:
                queued.append((obj, name, args))
            else:
                getattr(obj, name)(*args)

    class _Arg:
        def __init__(self, type_, value):
            self.value = type_(value)

    qtcore.QObject = _QObject
    qtcore.pyqtSignal = _Signal
    qtcore.pyqtSlot = lambda *a, **k: (lambda f: f)
    qtcore.QTimer = QTimer
    qtcore.QTime = QTime
    qtcore.QMetaObject = QMetaObject
    qtcore.Q_ARG = _Arg
    qtcore.Qt = types.SimpleNamespace(QueuedConnection=2)
    qtcore.QByteArray = bytes
    for name in ("QIODevice", "QThread", "QCoreApplication"):
        setattr(qtcore, name, _QObject)

    qtnet = types.ModuleType("PyQt5.QtNetwork")

    class QUdpSocket(_QObject):
        def __init__(self, *a, **k):
            self.readyRead = _BoundSignal()
            self.bound = None

        def bind(self, addr, port):
            self.bound = (addr, port)
            return True

        def hasPendingDatagrams(self):
            return False

        def close(self):
            self.bound = None

    qtnet.QUdpSocket = QUdpSocket
    qtnet.QHostAddress = _QObject
    qtw = types.ModuleType("PyQt5.QtWidgets")

    class QApplication(_QObject):
        def exec_(self):
            return 0

        def quit(self):
            pass

    qtw.QApplication = QApplication
    qt = types.ModuleType("PyQt5")
    qt.QtCore, qt.QtNetwork, qt.QtWidgets = qtcore, qtnet, qtw

    sio = types.ModuleType("flask_socketio")

    def emit(event, payload=None, **kw):
        log.emitted.append((event, payload))

    class SocketIO:
        def __init__(self, *a, **k):
            pass

        def on(self, *a, **k):
            return lambda f: f

        def emit(self, event, payload=None, **kw):
            emit(event, payload)

        def run(self, *a, **k):
            pass

    sio.SocketIO, sio.emit = SocketIO, emit

    ser = types.ModuleType("serial")

    class Serial:
        def __init__(self, *args, **kwargs):
            self._id = log.ports
            log.ports += 1
            self.is_open = True
            self.rx = bytearray()                       # what the board has sent; filled by the recorder
            log.add(OPEN, self._id, json.dumps({"args": list(args), "kwargs": kwargs}, sort_keys=True))

        def _open(self):
            if not self.is_open:
                raise OSError("port is closed")

        def write(self, data):
            self._open()
            log.add(WRITE, self._id, bytes(data))
            return len(data)

        def flush(self):
            self._open()
            log.add(FLUSH, self._id)

        @property
        def in_waiting(self):
            self._open()
            return len(self.rx)

        def read(self, size=1):
            self._open()
            out = bytes(self.rx[:size])
            del self.rx[:size]
            return out

        def reset_input_buffer(self):
            self._open()
            self.rx.clear()
            log.add(RESET_IN, self._id)

        def reset_output_buffer(self):
            self._open()
            log.add(RESET_OUT, self._id)

        def close(self):
            self.is_open = False
            log.add(CLOSE, self._id)

    ser.Serial = Serial
    return dict(zip(STAND_INS, (qt, qtcore, qtnet, qtw, sio, ser)))


def import_gui(log: Log | None = None, queued: list | None = None):
    """A fresh copy of scripts/fft_analyzer_gui.py, imported over the stand-ins.  The stand-ins stay in sys.modules (the
    module's methods import ``serial`` when they run) until the next call replaces them."""
    log = log if log is not None else Log()
    sys.modules.update(_make_modules(log, queued))
    spec = importlib.util.spec_from_file_location("fft_analyzer_gui", GUI_PATH)
    gui = importlib.util.module_from_spec(spec)
    with contextlib.redirect_stdout(io.StringIO()):
        spec.loader.exec_module(gui)
    gui.time = Clock(log)                                # the module's own clock: every time.time() / time.sleep() in it
    gui.receiver_state["fps_counters"]["time"] = log.t
    decode = gui.decode_mag_16iq_le

    def logging_decode(frame_bytes):
        log.frames.append(bytes(frame_bytes))
        return decode(frame_bytes)

    gui.decode_mag_16iq_le = logging_decode               # both receivers hand every complete frame to it
    return gui


def run_startup(gui):
    """Run the statements under ``if __name__ == '__main__':`` of the module in the module's namespace: its own start-up,
    with the stand-in QApplication (exec_ returns) and SocketIO (run returns)."""
    tree = ast.parse(open(GUI_PATH).read(), GUI_PATH)
    main = [n for n in tree.body if isinstance(n, ast.If) and isinstance(n.test, ast.Compare)
            and getattr(n.test.left, "id", None) == "__name__"]
    assert len(main) == 1
    exec(compile(ast.Module(body=main[0].body, type_ignores=[]), GUI_PATH, "exec"), gui.__dict__)


# ------------------------------------------------------------------------------------------------ recording
def samples() -> np.ndarray:
    """Three frames of 12-bit samples: a tone of its own per frame plus noise."""
    rng = np.random.default_rng(77)
    n = np.arange(N)
    bins = np.array([1234.5, 5000.25, 7900.0])
    x = 1500.0 * np.sin(2 * np.pi * bins[:, None] * n[None, :] / N + rng.uniform(0, 6.28, (3, 1))) \
        + 120.0 * rng.standard_normal((3, N))
    return np.clip(np.rint(x), -2048, 2047).astype(np.int16)


class Session:
    """One recorded session: a fresh import of the module, its log, and the helpers that stand for the user and the board."""

    def __init__(self, name: str, x: np.ndarray, mode: str = "UART", busy_main_thread: bool = False):
        from oracle import oracle as orc
        self.name, self.x, self.orc = name, x, orc
        self.log = Log()
        self.queued = [] if busy_main_thread else None
        self.gui = import_gui(self.log, self.queued)
        self.gui.web_config["comm_mode"] = mode
        self.frame_counters: list = []
        self.frame_shas: list = []

    def call(self, name: str, *args):
        """One user action: a handler of the module by name."""
        self.log.step(name if not args else f"{name} {json.dumps(args[0], sort_keys=True)}")
        with contextlib.redirect_stdout(io.StringIO()):
            getattr(self.gui, name)(*args)
            while self.queued:                              # busy main thread: the queued calls run after the handler
                obj, meth, a = self.queued.pop(0)
                getattr(obj, meth)(*a)

    def startup(self):
        self.log.step("startup")
        with contextlib.redirect_stdout(io.StringIO()):
            run_startup(self.gui)

    def pause(self, seconds: float):
        """The user waits."""
        self.log.step(f"pause {seconds:g} s")
        self.log.t += seconds
        self.log.add(PAUSE, -1, seconds * 1e3)

    def last_upload(self) -> np.ndarray:
        """The 12 coefficient bytes of the last 0xF1 upload in the write stream (zeros when a 0xFF came later or there is
        none): what the board holds."""
        c12, data, i = np.zeros(12, np.int8), self.log.written(), 0
        while i < len(data):
            if data[i] == 0xF1:
                c12 = np.frombuffer(data[i + 1:i + 13], np.int8).copy()
                i += 13
                continue
            if data[i] == 0xFF:
                c12 = np.zeros(12, np.int8)
            i += 1
        return c12

    def board_frames(self, n: int, cmd: int, c12=None) -> list:
        iq = self.orc.chain_q15(self.x[:n], None, 0, cmd, c12, None)
        return [iq[i].astype("<i2").tobytes() for i in range(n)]

    def _hand(self, frame: bytes) -> dict:
        """One frame into the current receiver the way its transport delivers it; returns the frame_data payload."""
        rx = self.gui.receiver_controller.current_receiver
        before = len(self.log.emitted)
        with contextlib.redirect_stdout(io.StringIO()):
            if isinstance(rx, self.gui.UartReceiver):
                for o in range(0, len(frame), 4096):        # the port never holds more than one read's worth
                    rx.ser.rx += frame[o:o + 4096]
                    self.log.t += 4096 * 10 / 230400.0      # the wire time of the chunk (8N1 at 230400 baud)
                    rx.read_timer.timeout.emit()            # -> read_data
            else:
                from fpga_real_time_fft_analyzer_amd import frames as fr
                self.log.t += 1.0 / 30.0 + 1e-3             # the board's frame rate
                for p in fr.frame_to_udp_payloads(frame):
                    rx.process_payload(p)
        got = [p for e, p in self.log.emitted[before:] if e == "frame_data"]
        assert len(got) == 1 and self.log.frames[-1] == frame
        return got[0]

    def receive(self, n: int, cmd: int = 0xB1, c12=None):
        """The board streams ``n`` frames under filter mode ``cmd`` (none when the RTL would be silent)."""
        rx = self.gui.receiver_controller.current_receiver
        uart = isinstance(rx, self.gui.UartReceiver)
        self.log.step(f"receive {n}")
        self.log.add(FRAMES, -1, (n, 0 if uart else 1))
        if n == 0 and uart:
            with contextlib.redirect_stdout(io.StringIO()):
                rx.read_timer.timeout.emit()
        for f in self.board_frames(n, cmd, c12) if n else []:
            p = self._hand(f)
            self.frame_counters.append((p["frames_received"], p["frames_displayed"]))
            self.frame_shas.append(sha(f))

    def sweep(self, n: int, cmd: int, c12=None) -> dict:
        """Every range of RANGES over ``n`` frames made under (cmd, c12), through the receiver that is running."""
        rx = self.gui.receiver_controller.current_receiver
        out = {"transport": 0 if isinstance(rx, self.gui.UartReceiver) else 1, "cmd": cmd,
               "c12": np.zeros(12, np.int8) if c12 is None else np.asarray(c12, np.int8), "frames": n,
               "peak_mag": np.zeros((8, n), np.float32), "peak_bin": np.zeros((8, n), np.int32),
               "len": np.zeros((8, n), np.int32), "bounds": np.zeros((8, 2), np.int32), "sha": [], "frame_sha": [],
               "received": np.zeros((8, n), np.int32), "displayed": np.zeros((8, n), np.int32)}
        frames_ = self.board_frames(n, cmd, c12)
        ramp = np.arange(N)
        events = len(self.log.events)
        for r, ((start, end), plots) in enumerate(zip(RANGES, RANGE_PLOTS)):
            with contextlib.redirect_stdout(io.StringIO()):
                self.gui.handle_apply_frequency_range({"freq_start": start, "freq_end": end, "plot_types": plots.split(",")})
            cut = self.gui.get_frequency_range_data(ramp)[1]
            out["bounds"][r] = (cut[0], cut[-1] + 1)
            assert np.array_equal(cut, np.arange(cut[0], cut[-1] + 1))
            re_, im_ = [], []
            for f, frame in enumerate(frames_):
                p = self._hand(frame)
                mag = np.asarray(p["data"]["magnitude"], np.float32)
                assert mag.astype(np.float64).tolist() == p["data"]["magnitude"]
                out["peak_mag"][r, f] = np.float32(p["peak_magnitude"])
                assert float(out["peak_mag"][r, f]) == p["peak_magnitude"]
                out["peak_bin"][r, f] = p["peak_bin"]
                out["len"][r, f] = len(p["frequency"])
                assert len(mag) == len(p["frequency"])
                out["received"][r, f], out["displayed"][r, f] = p["frames_received"], p["frames_displayed"]
                for key, dst in (("real", re_), ("imaginary", im_)):
                    if key in p["data"]:
                        a = np.asarray(p["data"][key], np.float64)
                        assert np.array_equal(a, a.astype(np.int16))
                        dst.append(a.astype(np.int16))
                    else:
                        assert key not in plots
                out["sha"].append(sha(mag.tobytes()))
                out["frame_sha"].append(sha(frame))
            if re_:
                out[f"re_{r}"] = np.stack(re_)
            if im_:
                out[f"im_{r}"] = np.stack(im_)
        assert len(self.log.events) == events               # receiving and changing the range write nothing
        out["sha"] = np.array(out["sha"]).reshape(8, n)
        out["frame_sha"] = np.array(out["frame_sha"]).reshape(8, n)
        return out

    def arrays(self, i: int) -> dict:
        ev, ms, blob, opens = [], [], bytearray(), []
        for kind, port, step, payload in self.log.events:
            a = b = 0
            gap = 0.0
            if kind == OPEN:
                a = len(opens)
                opens.append(payload)
            elif kind == WRITE:
                a, b = len(blob), len(payload)
                blob += payload
            elif kind in (GAP, TIMER, PAUSE):
                gap = payload
            elif kind == FRAMES:
                a, b = payload
            ev.append((kind, port, step, a, b))
            ms.append(gap)
        return {f"s{i}_steps": np.array(self.log.steps), f"s{i}_ev": np.array(ev, np.int32).reshape(-1, 5),
                f"s{i}_ms": np.array(ms, np.float64), f"s{i}_bytes": np.frombuffer(bytes(blob), np.uint8),
                f"s{i}_opens": np.array(opens), f"s{i}_counters": np.array(self.frame_counters, np.int32).reshape(-1, 2),
                f"s{i}_frame_sha": np.array(self.frame_shas, dtype="U64")}


DESIGNS = {  # what update_filter_config is given; the sections scipy returns before the pad / cut to two
    "lowpass4": {"filter_type": "lowpass", "filter_order": 4, "cutoff_freq": 10.0, "cutoff_freq2": 20.0, "sample_rate": 100.0},
    "lowpass2": {"filter_type": "lowpass", "filter_order": 2, "cutoff_freq": 10.0, "cutoff_freq2": 20.0, "sample_rate": 100.0},  # 1
    "highpass6": {"filter_type": "highpass", "filter_order": 6, "cutoff_freq": 5.0, "cutoff_freq2": 20.0, "sample_rate": 100.0},  # 3
    "bandpass2": {"filter_type": "bandpass", "filter_order": 2, "cutoff_freq": 10.0, "cutoff_freq2": 20.0, "sample_rate": 100.0},  # 2
}
FILTER_SESSION_ORDER = {"filters_uart": ["lowpass4", "lowpass2", "highpass6", "bandpass2"],
                        "filters_ethernet": ["bandpass2", "highpass6", "lowpass2", "lowpass4"]}


def _filters(s: Session):
    """Every design through the running receiver's upload path, each followed by custom / default / none; then custom once
    more, so that the session ends filtering with the last upload."""
    for d in FILTER_SESSION_ORDER[s.name]:
        s.call("handle_update_filter_config", DESIGNS[d])
        s.call("handle_apply_filter_to_fpga")
        for option in ("custom", "default", "none"):
            s.call("handle_set_filter_type", {"filter_option": option})
    s.call("handle_set_filter_type", {"filter_option": "custom"})


STAND_INS = ("PyQt5", "PyQt5.QtCore", "PyQt5.QtNetwork", "PyQt5.QtWidgets", "flask_socketio", "serial")


def record_all():
    """Run every session.  Returns the dict of arrays of g7_gui_sessions.npz; sys.modules is left as it was found."""
    before = {name: sys.modules.get(name) for name in STAND_INS}
    try:
        return _record_all()
    finally:
        for name, mod in before.items():
            if mod is None:
                sys.modules.pop(name, None)
            else:
                sys.modules[name] = mod


def _record_all():
    x = samples()
    sessions, sweeps = [], []

    # 1. start-up in UART mode, start, three frames
    s = Session("uart_startup", x, "UART")
    s.startup()
    s.call("handle_start_receiver")
    s.receive(3, 0xB1)
    sessions.append(s)
    sweeps.append((0, s.sweep(3, 0xB1)))

    # 2. the same in Ethernet mode; then the default filter, through a temporary port like every command there
    s = Session("ethernet_startup", x, "ETHERNET")
    s.startup()
    s.call("handle_start_receiver")
    s.receive(3, 0xB1)
    s.call("handle_set_filter_type", {"filter_option": "default"})
    sessions.append(s)
    sweeps.append((1, s.sweep(3, 0x00)))

    # 3. mode switches with a receiver running: the queued stop_receiver has run when handle_set_mode looks at the
    #    receiver, so the three 0xFF go through a temporary port
    s = Session("mode_switch", x, "UART")
    s.startup()
    s.call("handle_start_receiver")
    s.receive(1, 0xB1)
    for mode in ("ETHERNET", "UART"):
        s.call("handle_update_config", {"comm_mode": mode})
        s.call("handle_set_mode")
        s.call("handle_start_receiver")
        s.receive(1, 0xB1)
    sessions.append(s)

    # 3b. the same switches with the Qt thread busy: the queued calls run after the handler, so the UartReceiver is still
    #     there and force_mode_reset writes the three 0xFF on the live port
    s = Session("mode_switch_busy_main_thread", x, "UART", busy_main_thread=True)
    s.startup()
    s.call("handle_start_receiver")
    s.receive(1, 0xB1)
    for mode in ("ETHERNET", "UART"):
        s.call("handle_update_config", {"comm_mode": mode})
        s.call("handle_set_mode")
        s.call("handle_start_receiver")
        s.receive(1, 0xB1)
    sessions.append(s)

    # 4. filter uploads through the live UartReceiver, and through the temporary port of the Ethernet mode
    for name, mode in (("filters_uart", "UART"), ("filters_ethernet", "ETHERNET")):
        s = Session(name, x, mode)
        s.startup()
        s.call("handle_start_receiver")
        _filters(s)
        c12 = s.last_upload()
        s.receive(2, 0xA1, c12)
        sessions.append(s)
        sweeps.append((len(sessions) - 1, s.sweep(2, 0xA1, c12)))

    # 5. resets: accepted, swallowed inside the 2 s cool-down, accepted after it; then the custom filter with nothing
    #    uploaded since.  The reset leaves the board on Ethernet (imp/sequ2.vhd:85-86) and the GUI sends no mode byte after it:
    #    the start that follows reaches the Ethernet machine and the UART stays silent.
    s = Session("reset_cooldown", x, "UART")
    s.startup()
    s.call("handle_update_filter_config", DESIGNS["lowpass4"])
    s.call("handle_apply_filter_to_fpga")
    s.call("handle_set_filter_type", {"filter_option": "custom"})
    s.call("handle_fpga_reset")
    s.pause(0.5)
    s.call("handle_fpga_reset")
    s.pause(2.0)
    s.call("handle_fpga_reset")
    s.call("handle_set_filter_type", {"filter_option": "custom"})
    s.call("handle_start_receiver")
    s.receive(0)
    assert not s.last_upload().any()
    sessions.append(s)
    sweeps.append((len(sessions) - 1, s.sweep(1, 0xA1, s.last_upload())))

    out = {"x": x, "ranges": np.array(RANGES, np.float64), "range_plots": np.array(RANGE_PLOTS),
           "session_names": np.array([s.name for s in sessions])}
    for i, s in enumerate(sessions):
        out.update(s.arrays(i))
    out["sweep_session"] = np.array([i for i, _ in sweeps], np.int32)
    for key, dt in (("transport", np.int32), ("cmd", np.uint8), ("frames", np.int32)):
        out[f"sweep_{key}"] = np.array([w[key] for _, w in sweeps], dt)
    out["sweep_c12"] = np.stack([w["c12"] for _, w in sweeps]).astype(np.int8)
    for j, (_, w) in enumerate(sweeps):
        for key, v in w.items():
            if key not in ("transport", "cmd", "c12", "frames"):
                out[f"w{j}_{key}"] = v
    return out


def write(path: str = FIXTURE) -> int:
    arrays = record_all()
    assert all(a.dtype != object for a in arrays.values())
    np.savez_compressed(path, **arrays)
    return os.path.getsize(path)


if __name__ == "__main__":
    print(f"{FIXTURE}: {write() / 1024:.0f} KiB")
