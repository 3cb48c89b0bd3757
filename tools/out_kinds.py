#!/usr/bin/env python3
"""Diagnostic: time of the fused float chain for each output kind at B = 4096, in modes 0xA1 (the G2 Butterworth) and
0xB1, in one process.  The kinds alternate round by round (each round: warm-up, then a timed train of stream-ordered
calls over 4 rotating buffer pairs; wall time per call), and the kernel's own time comes from the launch-timing ring
(sa_set_profiling).  usage: out_kinds.py [--rounds R] [--calls C]   (GPU)"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fpga_real_time_fft_analyzer_amd.chain import SpectrumChain  # noqa: E402

KINDS = ("mag_full", "mag_half", "spec_half", "time", "marker")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--calls", type=int, default=60)
    a = ap.parse_args()
    B, N, R = 4096, 16384, 4
    ch = SpectrumChain(0)
    ch.load_sos(np.load(os.path.join(ROOT, "tests", "golden", "g2_config1.npz"))["sos"])
    gen = torch.Generator(device="cuda").manual_seed(1)
    xs = [torch.randn(B, N, generator=gen, device="cuda") for _ in range(R)]
    outs = {k: [ch.process_f32(xs[r], out_kind=k) for r in range(R)] for k in KINDS}
    for mode in (0xA1, 0xB1):
        ch.set_filter_mode(mode)
        wall = {k: [] for k in KINDS}
        for _ in range(a.rounds):
            for kind in KINDS:
                for i in range(5):
                    ch.process_f32(xs[i % R], out=outs[kind][i % R], out_kind=kind)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(a.calls):
                    ch.process_f32(xs[i % R], out=outs[kind][i % R], out_kind=kind)
                torch.cuda.synchronize()
                wall[kind].append((time.perf_counter() - t0) / a.calls)
        kern = {}
        ch.set_profiling(a.calls)
        for kind in KINDS:
            for i in range(a.calls):
                ch.process_f32(xs[i % R], out=outs[kind][i % R], out_kind=kind)
            kern[kind] = float(np.median(ch.profile_read(a.calls))) * 1e-3
        ch.set_profiling(0)
        for kind in KINDS:
            dt = float(np.median(wall[kind]))
            nbytes = B * N * 4 + outs[kind][0].numel() * outs[kind][0].element_size()
            print(f"mode 0x{mode:02X} {kind:10s} {dt*1e6:7.1f} us  {B/dt/1e6:6.2f} M frames/s  {nbytes/dt/1e12:5.2f} TB/s"
                  f"  kernel {kern[kind]*1e6:7.1f} us  (wall: median of {a.rounds} alternating rounds of {a.calls} calls,"
                  f" spread {min(wall[kind])*1e6:.1f}-{max(wall[kind])*1e6:.1f}; kernel: median of {a.calls} timed calls)",
                  flush=True)
    ch.close()


if __name__ == "__main__":
    main()
