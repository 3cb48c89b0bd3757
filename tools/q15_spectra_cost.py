#!/usr/bin/env python3
"""Cost of the full-resolution spectra over groups of A frames (include/specan_ext.h; SpectrumChain.spectra_q15 and
fold_iq_q15) at B = 4096, A = 4, 16 and 128, in modes 0xB1, 0x00 and 0xA2.  The columns of a part alternate in one process over
several rounds (each round: warm-up calls, then a timed train); a ratio is read beside the spread of its columns' own round
medians, and never against a stored number.
Part 1, fold cost.  (a) device time per call from the launches' own events (sa_set_profiling): the 'iq' call -- the parent's
kernels, the yardstick -- the spectra call, which is that call into a workspace plus the fold, and the fold alone.  (b) the fold
alone against a device-to-device copy_ of the same IQ tensor, both timed by events around the one operation on the same
stream: the copy moves 2 x B x 65536 bytes, the fold (1 + 2 / A) x B x 65536.
Part 2, against what a user does today on the device: process_q15('iq') followed by a torch reduction to the same records
(whether its bits are the same is printed, not assumed), events on the same stream.
Part 3, with the result copied to pinned host memory behind each call: spectra against 'mag' + copy (bound: the byte ratio
A / 2) and against traces_q15(16, group=A).
usage: q15_spectra_cost.py [--rounds R] [--calls C] [--batch B]   (GPU)"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fpga_real_time_fft_analyzer_amd.chain import SpectrumChain  # noqa: E402

GROUPS = (4, 16, 128)
MODES = (0xB1, 0x00, 0xA2)
N = 16384


def spread(v):
    return f"{min(v):.1f}-{max(v):.1f} ({max(v) / min(v):.3f})"


def torch_records(iq, A):
    """the records of spectra_q15 by stock torch kernels on the IQ tensor: separate multiply and add kernels (no contraction),
    the root after the maximum, the power summed in int64 and converted once"""
    B = iq.shape[0]
    re, im = iq[..., 0], iq[..., 1]
    rf, jf = re.float(), im.float()
    s = (rf * rf + jf * jf).view(B // A, A, N).amax(1)
    rl, jl = re.long(), im.long()
    p = (rl * rl + jl * jl).view(B // A, A, N).sum(1)
    return torch.stack((s.sqrt(), p.float()), dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--calls", type=int, default=16)
    ap.add_argument("--batch", type=int, default=4096)
    a = ap.parse_args()
    B = a.batch
    from scipy import signal
    sos14 = np.rint(16384.0 * np.concatenate([signal.butter(2, wc, output="sos") for wc in (0.35, 0.45, 0.55, 0.65, 0.75, 0.85)]))
    sos14 = np.ascontiguousarray(sos14.astype(np.int16))
    rng = np.random.default_rng(5)
    n = np.arange(N)
    D = min(B, 256)                                            # tones + noise, 12 bits: 256 distinct frames, repeated
    x = 1500.0 * np.sin(2 * np.pi * rng.uniform(0.01, 0.45, (D, 1)) * n) + 200.0 * rng.standard_normal((D, N))
    xd = torch.from_numpy(np.clip(np.rint(x), -2048, 2047).astype(np.int16)).cuda().repeat((B + D - 1) // D, 1)[:B].contiguous()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]

    def by_events(fn):
        """median us of `fn` over a train of a.calls, each between its own pair of events on the current stream"""
        fn()
        torch.cuda.synchronize()
        for s, e in ev:
            s.record()
            fn()
            e.record()
        torch.cuda.synchronize()
        return float(np.median([s.elapsed_time(e) for s, e in ev])) * 1e3

    print(f"B = {B}, {a.rounds} alternating rounds of {a.calls} timed calls per column; us per call", flush=True)
    with SpectrumChain(0) as ch:
        ch.load_sos_q14(sos14)
        ch.reserve(B)
        iq = ch.process_q15(xd)
        iq2 = torch.empty_like(iq)
        mag = ch.process_q15(xd, out_kind="mag")
        rec = {A: ch.spectra_q15(xd, A) for A in GROUPS}       # the first call grows the workspace of IQ frames
        tr = {A: ch.traces_q15(xd, bucket=16, group=A) for A in GROUPS}
        host = torch.empty(mag.numel() * 4, dtype=torch.uint8).pin_memory()
        iq_bytes = B * 65536
        print(f"IQ tensor {iq_bytes >> 20} MiB; result bytes per input frame: iq 65536  mag 65536  "
              + "  ".join(f"spectra A{A} {131072 // A}" for A in GROUPS) + "  " + "  ".join(f"W16xA{A} {8192 // A}" for A in GROUPS), flush=True)
        for mode in MODES:
            ch.set_filter_mode(mode)
            ch.process_q15(xd, out=iq)
            for A in GROUPS:                                       # the call is the fold of the IQ call, and what torch makes of it
                ch.spectra_q15(xd, A, out=rec[A])
                assert torch.equal(ch.fold_iq_q15(iq, A).view(torch.int32), rec[A].view(torch.int32)), (hex(mode), A)
                t = torch_records(iq, A)
                dp = int((t[..., 0].view(torch.int32) != rec[A][..., 0].view(torch.int32)).sum())
                dw = int((t[..., 1].view(torch.int32) != rec[A][..., 1].view(torch.int32)).sum())
                print(f"mode 0x{mode:02X} A{A}: torch reduction differs from the records in {dp} peak and {dw} power words "
                      f"of {rec[A].numel() // 2}", flush=True)
                del t
            # part 1a: device time of the calls, from their own events
            cols = ["iq"] + [f"spectra A{A}" for A in GROUPS] + [f"fold A{A}" for A in GROUPS]
            calls = {"iq": lambda: ch.process_q15(xd, out=iq)}
            for A in GROUPS:
                calls[f"spectra A{A}"] = lambda A=A: ch.spectra_q15(xd, A, out=rec[A])
                calls[f"fold A{A}"] = lambda A=A: ch.fold_iq_q15(iq, A, out=rec[A])
            ch.set_profiling(a.calls)
            med = {k: [] for k in cols}
            for _ in range(a.rounds):
                for k in cols:
                    for _ in range(2):
                        calls[k]()
                    torch.cuda.synchronize()
                    for _ in range(a.calls):
                        calls[k]()
                    ms = ch.profile_read(a.calls)
                    assert len(ms) == a.calls
                    med[k].append(float(np.median(ms)) * 1e3)
            ch.set_profiling(0)
            c = {k: float(np.median(med[k])) for k in cols}
            print(f"mode 0x{mode:02X} device time : " + "  ".join(f"{k} {c[k]:7.1f}" for k in cols), flush=True)
            print("          spectra / iq: " + "  ".join(f"A{A} {c[f'spectra A{A}'] / c['iq']:.3f}" for A in GROUPS)
                  + "   spectra - iq - fold [us]: " + "  ".join(f"A{A} {c[f'spectra A{A}'] - c['iq'] - c[f'fold A{A}']:+.1f}" for A in GROUPS), flush=True)
            print("          fold alone, input bytes / time: "
                  + "  ".join(f"A{A} {iq_bytes / c[f'fold A{A}'] / 1e6:.2f} TB/s" for A in GROUPS), flush=True)
            print("          round medians: " + "  ".join(f"{k} {spread(med[k])}" for k in cols), flush=True)
            # part 1b: the fold alone against a device-to-device copy of the same tensor, events around the one operation
            cols = ["copy_"] + [f"fold A{A}" for A in GROUPS]
            calls["copy_"] = lambda: iq2.copy_(iq)
            med = {k: [] for k in cols}
            for _ in range(a.rounds):
                for k in cols:
                    med[k].append(by_events(calls[k]))
            c = {k: float(np.median(med[k])) for k in cols}
            print(f"mode 0x{mode:02X} by events   : " + "  ".join(f"{k} {c[k]:7.1f}" for k in cols), flush=True)
            print("          fold / copy_ (the condition: at most 1; bytes moved, fold / copy: "
                  + " ".join(f"{(1 + 2 / A) / 2:.3f}" for A in GROUPS) + "): "
                  + "  ".join(f"A{A} {c[f'fold A{A}'] / c['copy_']:.3f}" for A in GROUPS), flush=True)
            print("          round medians: " + "  ".join(f"{k} {spread(med[k])}" for k in cols), flush=True)
            # part 2: the call against the IQ call and a torch reduction
            cols = [f"{w} A{A}" for A in GROUPS for w in ("spectra", "iq+torch")]
            for A in GROUPS:
                calls[f"iq+torch A{A}"] = lambda A=A: torch_records(ch.process_q15(xd, out=iq), A)
            med = {k: [] for k in cols}
            for _ in range(a.rounds):
                for k in cols:
                    med[k].append(by_events(calls[k]))
            c = {k: float(np.median(med[k])) for k in cols}
            print(f"mode 0x{mode:02X} on the device: " + "  ".join(f"{k} {c[k]:7.1f}" for k in cols), flush=True)
            print("          iq+torch / spectra: " + "  ".join(f"A{A} {c[f'iq+torch A{A}'] / c[f'spectra A{A}']:.2f}" for A in GROUPS), flush=True)
            print("          round medians: " + "  ".join(f"{k} {spread(med[k])}" for k in cols), flush=True)
            torch.cuda.empty_cache()
            # part 3: call + copy of the result to pinned host memory
            def with_copy(fn, t):
                src, dst = t.view(-1).view(torch.uint8), host[:t.numel() * t.element_size()]
                return lambda: (fn(), dst.copy_(src, non_blocking=True))

            cols = ["mag"] + [f"{w} A{A}" for A in GROUPS for w in ("spectra", "W16x")]
            calls3 = {"mag": with_copy(lambda: ch.process_q15(xd, out=mag, out_kind="mag"), mag)}
            for A in GROUPS:
                calls3[f"spectra A{A}"] = with_copy(calls[f"spectra A{A}"], rec[A])
                calls3[f"W16x A{A}"] = with_copy(lambda A=A: ch.traces_q15(xd, bucket=16, group=A, out=tr[A]), tr[A])
            med = {k: [] for k in cols}
            for _ in range(a.rounds):
                for k in cols:
                    med[k].append(by_events(calls3[k]))
            c = {k: float(np.median(med[k])) for k in cols}
            print(f"mode 0x{mode:02X} call + copy  : " + "  ".join(f"{k} {c[k]:7.1f}" for k in cols), flush=True)
            print("          mag / spectra (bound: the byte ratio A / 2): "
                  + "  ".join(f"A{A} {c['mag'] / c[f'spectra A{A}']:.2f}" for A in GROUPS)
                  + "   spectra / W16x of the same A: " + "  ".join(f"A{A} {c[f'spectra A{A}'] / c[f'W16x A{A}']:.2f}" for A in GROUPS), flush=True)
            print("          round medians: " + "  ".join(f"{k} {spread(med[k])}" for k in cols), flush=True)


if __name__ == "__main__":
    main()
