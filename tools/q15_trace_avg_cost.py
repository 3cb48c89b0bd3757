#!/usr/bin/env python3
"""Cost of the grouped trace (SA_Q15_TRACE_AVG_KIND, SpectrumChain.traces_q15(group=A)) beside the plain trace at B = 4096:
the plain trace at W = 16 and W = 64 and the grouped kind at the same W with A = 4, 16 and 128, alternating in one process
over several rounds (each round: warm-up calls, then a timed train), in modes 0xB1, 0x00 and 0xA2.
Part 1: device time per call from the launches' own events (sa_set_profiling): for the grouped kind it spans the FFT launch
(with the cascade in front of it in 0x00 / 0xA2) and the fold launch behind it.
Part 2: the same calls followed by the copy of the result to pinned host memory, timed by events around call + copy on
the caller's stream.  The bound on the gain there is the byte ratio of the results, A, quoted on the line.
Part 3 (--ab LIB, a `make -C csrc ab NAME=nt EXTRA=-DSA_FX_RAW_NT` build): the grouped calls of part 1 through the product
library and through LIB alternately, on handles of their own -- plain against nontemporal stores of the partial records.
The yardstick is the plain-trace column of the same W in the same run: compare within a line, never against a stored number,
and read a ratio beside the spread of the columns' own round medians.
usage: q15_trace_avg_cost.py [--rounds R] [--calls C] [--batch B] [--ab libspecan_ab_nt.so]   (GPU)"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fpga_real_time_fft_analyzer_amd import abi  # noqa: E402
from fpga_real_time_fft_analyzer_amd.chain import SpectrumChain  # noqa: E402

WIDTHS = (16, 64)
GROUPS = (4, 16, 128)
KINDS = tuple((W, A) for W in WIDTHS for A in (None,) + GROUPS)
MODES = (0xB1, 0x00, 0xA2)


def name(kind):
    W, A = kind
    return f"W{W}" if A is None else f"W{W}xA{A}"


def spread(v):
    return f"{min(v):.1f}-{max(v):.1f} ({max(v) / min(v):.3f})"


class RawHandle:
    """A handle of another build of the library (an A/B build is never loaded by the package): the few calls timed here."""

    def __init__(self, path, sos14):
        self.L = L = C.CDLL(path)
        for fn, (restype, argtypes) in abi.SIGNATURES.items():
            getattr(L, fn).restype, getattr(L, fn).argtypes = restype, argtypes
        self.h = C.c_void_p()
        assert L.sa_create(0, C.byref(self.h)) == 0
        assert L.sa_load_sos_q14(self.h, sos14.ctypes.data_as(C.POINTER(C.c_int16)), sos14.shape[0]) == 0

    def traces(self, x, W, A, out):
        code = abi.SA_Q15_TRACE_AVG_KIND(W.bit_length() - 1, A.bit_length() - 1)
        rc = self.L.sa_process_q15_out(self.h, x.data_ptr(), out.data_ptr(), x.shape[0], code, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, self.L.sa_last_error(self.h)

    def times(self, n):
        buf = (C.c_float * n)()
        assert self.L.sa_profile_read(self.h, buf, n) == n
        return list(buf)

    def close(self):
        self.L.sa_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--calls", type=int, default=16)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--ab", default=None, help="another build of the library, relative to the package directory")
    a = ap.parse_args()
    B, N = a.batch, 16384
    from scipy import signal
    # six Q2.14 sections that pass signal: second-order Butterworth low-passes of unity DC gain
    sos14 = np.rint(16384.0 * np.concatenate([signal.butter(2, wc, output="sos") for wc in (0.35, 0.45, 0.55, 0.65, 0.75, 0.85)]))
    sos14 = np.ascontiguousarray(sos14.astype(np.int16))
    rng = np.random.default_rng(5)
    n = np.arange(N)
    # tones + noise in the ADC's range, quantised to 12 bits: 256 distinct frames, repeated up to the batch
    D = min(B, 256)
    x = 1500.0 * np.sin(2 * np.pi * rng.uniform(0.01, 0.45, (D, 1)) * n) + 200.0 * rng.standard_normal((D, N))
    xi = np.clip(np.rint(x), -2048, 2047).astype(np.int16)
    xd = torch.from_numpy(xi).cuda().repeat((B + D - 1) // D, 1)[:B].contiguous()
    print(f"B = {B}, {a.rounds} alternating rounds of {a.calls} timed calls per kind; us per call; W16 / W64: the plain trace, "
          f"WwxAa: groups of a frames", flush=True)
    with SpectrumChain(0) as ch:
        ch.load_sos_q14(sos14)
        ch.reserve(B)

        def call(kind, out=None):
            return ch.traces_q15(xd, bucket=kind[0], out=out, group=kind[1])

        outs = {k: call(k) for k in KINDS}                     # the first grouped calls grow the workspace of partial records
        nbytes = {k: outs[k].numel() * outs[k].element_size() for k in KINDS}
        host = torch.empty(max(nbytes.values()), dtype=torch.uint8).pin_memory()
        print("result bytes per input frame: " + "  ".join(f"{name(k)} {nbytes[k] / B:g}" for k in KINDS), flush=True)
        print("partial records per call: " + "  ".join(f"W{W} {B * (N // W) * 16 >> 20} MiB" for W in WIDTHS), flush=True)
        for mode in MODES:
            ch.set_filter_mode(mode)
            # the grouped kind is the reduction of the plain trace of the same call sequence (checked once per mode)
            for W in WIDTHS:
                t = call((W, None), outs[W, None])
                for A in GROUPS:
                    g = call((W, A), outs[W, A])
                    assert torch.equal(g[..., 0], t[..., 0].reshape(B // A, A, N // W).amax(1)), (hex(mode), W, A)
            # part 1: device time of the call
            ch.set_profiling(a.calls)
            med = {k: [] for k in KINDS}
            for _ in range(a.rounds):
                for k in KINDS:
                    for _ in range(2):
                        call(k, outs[k])
                    torch.cuda.synchronize()
                    for _ in range(a.calls):
                        call(k, outs[k])
                    ms = ch.profile_read(a.calls)
                    assert len(ms) == a.calls
                    med[k].append(float(np.median(ms)) * 1e3)
            ch.set_profiling(0)
            c = {k: float(np.median(med[k])) for k in KINDS}
            print(f"mode 0x{mode:02X} device time : " + "  ".join(f"{name(k)} {c[k]:7.1f}" for k in KINDS), flush=True)
            print("          grouped / plain of the same W: "
                  + "  ".join(f"{name((W, A))} {c[W, A] / c[W, None]:.3f}" for W in WIDTHS for A in GROUPS), flush=True)
            print("          round medians: " + "  ".join(f"{name(k)} {spread(med[k])}" for k in KINDS), flush=True)
            # part 2: call + copy of the result to pinned host memory
            med = {k: [] for k in KINDS}
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]
            for _ in range(a.rounds):
                for k in KINDS:
                    src, dst = outs[k].view(-1).view(torch.uint8), host[:nbytes[k]]
                    call(k, outs[k])
                    dst.copy_(src, non_blocking=True)
                    torch.cuda.synchronize()
                    for s, e in ev:
                        s.record()
                        call(k, outs[k])
                        dst.copy_(src, non_blocking=True)
                        e.record()
                    torch.cuda.synchronize()
                    med[k].append(float(np.median([s.elapsed_time(e) for s, e in ev])) * 1e3)
            c = {k: float(np.median(med[k])) for k in KINDS}
            print(f"mode 0x{mode:02X} call + copy  : " + "  ".join(f"{name(k)} {c[k]:7.1f}" for k in KINDS), flush=True)
            print("          plain / grouped of the same W (bound: the byte ratio A): "
                  + "  ".join(f"{name((W, A))} {c[W, None] / c[W, A]:.2f}" for W in WIDTHS for A in GROUPS), flush=True)
            print("          round medians: " + "  ".join(f"{name(k)} {spread(med[k])}" for k in KINDS), flush=True)
    if a.ab is None:
        return
    # part 3: two builds, the grouped kinds alone, device time
    libs = {"product": RawHandle(abi.LIB_PATH, sos14), a.ab: RawHandle(os.path.join(os.path.dirname(abi.LIB_PATH), a.ab), sos14)}
    grouped = [k for k in KINDS if k[1] is not None]
    outs = {k: torch.empty((B // k[1], N // k[0], 2), dtype=torch.float32, device="cuda") for k in grouped}
    for mode in MODES:
        med = {(lib, k): [] for lib in libs for k in grouped}
        first = {}
        for h in libs.values():
            assert h.L.sa_set_filter_mode(h.h, mode) == 0 and h.L.sa_set_profiling(h.h, a.calls) == 0
        for rnd in range(a.rounds):
            for k in grouped:
                for lib, h in (list(libs.items()) if rnd % 2 == 0 else list(libs.items())[::-1]):
                    for _ in range(2):
                        h.traces(xd, k[0], k[1], outs[k])
                    torch.cuda.synchronize()
                    if rnd == 0:
                        assert torch.equal(first.setdefault(k, outs[k].clone()), outs[k]), (lib, k)
                    for _ in range(a.calls):
                        h.traces(xd, k[0], k[1], outs[k])
                    med[lib, k].append(float(np.median(h.times(a.calls))) * 1e3)
        for h in libs.values():
            assert h.L.sa_set_profiling(h.h, 0) == 0
        for lib in libs:
            print(f"mode 0x{mode:02X} {lib:24s}: " + "  ".join(f"{name(k)} {np.median(med[lib, k]):7.1f}" for k in grouped), flush=True)
            print("          round medians: " + "  ".join(f"{name(k)} {spread(med[lib, k])}" for k in grouped), flush=True)
        print(f"mode 0x{mode:02X} {a.ab} / product: "
              + "  ".join(f"{name(k)} {np.median(med[a.ab, k]) / np.median(med['product', k]):.3f}" for k in grouped), flush=True)
    for h in libs.values():
        h.close()


if __name__ == "__main__":
    main()
