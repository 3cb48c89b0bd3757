#!/usr/bin/env python3
"""Cost of the integer chain's display trace (SA_Q15_TRACE_KIND, SpectrumChain.traces_q15) beside its other output kinds at
B = 4096: 'iq', 'mag', 'marker' and the trace at W = 16 and W = 64, alternating in one process over several rounds (each
round: warm-up calls, then a timed train), in modes 0xB1, 0x00 and 0xA2.
Part 1: device time per call from the launches' own events (sa_set_profiling).
Part 2: the same calls followed by the copy of the result to pinned host memory, timed by events around call + copy on
the caller's stream -- what a host that wants the spectra pays.  The bound on the gain there is the byte ratio of the
results (mag / trace at W = 16: 8x), quoted on the line.
Every column is the reference of its own run: compare within a line, never against a stored number, and read a ratio
beside the spread of the columns' own round medians.
usage: q15_trace_cost.py [--rounds R] [--calls C] [--batch B]   (GPU)"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fpga_real_time_fft_analyzer_amd.chain import SpectrumChain  # noqa: E402

KINDS = ("iq", "mag", "marker", "trace16", "trace64")


def call(ch, kind, x, out=None):
    if kind.startswith("trace"):
        return ch.traces_q15(x, bucket=int(kind[5:]), out=out)
    return ch.process_q15(x, out=out, out_kind=kind)


def spread(v):
    return f"{min(v):.1f}-{max(v):.1f} ({max(v) / min(v):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--calls", type=int, default=16)
    ap.add_argument("--batch", type=int, default=4096)
    a = ap.parse_args()
    B, N = a.batch, 16384
    from scipy import signal
    # six Q2.14 sections that pass signal: second-order Butterworth low-passes of unity DC gain
    sos14 = np.rint(16384.0 * np.concatenate([signal.butter(2, wc, output="sos") for wc in (0.35, 0.45, 0.55, 0.65, 0.75, 0.85)]))
    sos14 = sos14.astype(np.int16)
    rng = np.random.default_rng(5)
    n = np.arange(N)
    # tones + noise in the ADC's range, quantised to 12 bits: 256 distinct frames, repeated up to the batch
    D = min(B, 256)
    x = 1500.0 * np.sin(2 * np.pi * rng.uniform(0.01, 0.45, (D, 1)) * n) + 200.0 * rng.standard_normal((D, N))
    xi = np.clip(np.rint(x), -2048, 2047).astype(np.int16)
    xd = torch.from_numpy(xi).cuda().repeat((B + D - 1) // D, 1)[:B].contiguous()
    print(f"B = {B}, {a.rounds} alternating rounds of {a.calls} timed calls per kind; us per call", flush=True)
    with SpectrumChain(0) as ch:
        ch.load_sos_q14(sos14)
        ch.reserve(B)
        outs = {k: call(ch, k, xd) for k in KINDS}
        nbytes = {k: outs[k].numel() * outs[k].element_size() for k in KINDS}
        host = torch.empty(max(nbytes.values()), dtype=torch.uint8).pin_memory()
        hosts = {k: host[:nbytes[k]] for k in KINDS}
        print("result bytes per frame: " + "  ".join(f"{k} {nbytes[k] // B}" for k in KINDS), flush=True)
        for mode in (0xB1, 0x00, 0xA2):
            ch.set_filter_mode(mode)
            # the trace is the reduction of the mag output of the same call sequence (checked once per mode)
            m = call(ch, "mag", xd, outs["mag"])
            for W in (16, 64):
                t = call(ch, f"trace{W}", xd, outs[f"trace{W}"])
                assert torch.equal(t[..., 0], m.view(B, N // W, W).amax(-1)), (hex(mode), W)
            # part 1: device time of the call
            ch.set_profiling(a.calls)
            med = {k: [] for k in KINDS}
            for _ in range(a.rounds):
                for k in KINDS:
                    for _ in range(2):
                        call(ch, k, xd, outs[k])
                    torch.cuda.synchronize()
                    for _ in range(a.calls):
                        call(ch, k, xd, outs[k])
                    ms = ch.profile_read(a.calls)
                    assert len(ms) == a.calls
                    med[k].append(float(np.median(ms)) * 1e3)
            ch.set_profiling(0)
            c = {k: float(np.median(med[k])) for k in KINDS}
            print(f"mode 0x{mode:02X} device time : " + "  ".join(f"{k} {c[k]:7.1f}" for k in KINDS)
                  + f"   trace16/mag {c['trace16'] / c['mag']:.3f}  trace16/iq {c['trace16'] / c['iq']:.3f}"
                  + f"  trace64/mag {c['trace64'] / c['mag']:.3f}", flush=True)
            print("          round medians: " + "  ".join(f"{k} {spread(med[k])}" for k in KINDS), flush=True)
            # part 2: call + copy of the result to pinned host memory
            med = {k: [] for k in KINDS}
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]
            for _ in range(a.rounds):
                for k in KINDS:
                    src = outs[k].view(-1).view(torch.uint8)
                    call(ch, k, xd, outs[k])
                    hosts[k].copy_(src, non_blocking=True)
                    torch.cuda.synchronize()
                    for s, e in ev:
                        s.record()
                        call(ch, k, xd, outs[k])
                        hosts[k].copy_(src, non_blocking=True)
                        e.record()
                    torch.cuda.synchronize()
                    med[k].append(float(np.median([s.elapsed_time(e) for s, e in ev])) * 1e3)
            c = {k: float(np.median(med[k])) for k in KINDS}
            print(f"mode 0x{mode:02X} call + copy  : " + "  ".join(f"{k} {c[k]:7.1f}" for k in KINDS)
                  + f"   mag/trace16 {c['mag'] / c['trace16']:.2f} (byte ratio {nbytes['mag'] / nbytes['trace16']:.0f})"
                  + f"  mag/trace64 {c['mag'] / c['trace64']:.2f} (byte ratio {nbytes['mag'] / nbytes['trace64']:.0f})", flush=True)
            print("          round medians: " + "  ".join(f"{k} {spread(med[k])}" for k in KINDS), flush=True)


if __name__ == "__main__":
    main()
