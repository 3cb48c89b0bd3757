#!/usr/bin/env python3
"""Cost of the float fold (include/specan_fold.h; SpectrumChain.fold_mag_f32 and spectra_f32) at B = 4096, in filter mode 0xB1.
Every column is timed between a pair of events on the current stream around the one operation; the columns of a part alternate
in one process over several rounds (each round: a warm-up call, then a timed train), and a ratio is read beside the spread of
its columns' own round medians, never against a stored number.
Part 1: the fold alone at (A, W) = (4,1), (16,1), (128,1), (1,16), (16,16) against a device-to-device copy_ of the same 256 MiB
        magnitude tensor: the copy moves 2 x B x 65536 bytes, the fold (1 + 2 / (A W)) x B x 65536.  1a rotates every column
        over three equal input tensors (768 MiB), so that no call finds its input in the 256 MiB Infinity Cache; 1b re-reads
        one tensor call after call, which a fold whose input was just written by the chain comes closer to.
Part 2: spectra_f32 against process_f32('mag_full'), the call it contains.
Part 3: both with the result copied to pinned host memory behind the call, against 'mag_full' plus its copy.
usage: fold_f32_time.py [--rounds R] [--calls C] [--batch B] [--out FILE]   (GPU; FILE defaults to profiles/r15_f32_fold.txt)"""
import argparse
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fpga_real_time_fft_analyzer_amd import frames  # noqa: E402
from fpga_real_time_fft_analyzer_amd.chain import SpectrumChain  # noqa: E402

PAIRS = ((4, 1), (16, 1), (128, 1), (1, 16), (16, 16))
N = 16384


def spread(v):
    return f"{min(v):.1f}-{max(v):.1f} ({max(v) / min(v):.3f})"


def name(p):
    return f"A{p[0]}xW{p[1]}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--calls", type=int, default=16)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_f32_fold.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    B = a.batch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(5)
    n = np.arange(N)
    D = min(B, 256)                                            # tones + noise: 256 distinct frames, repeated
    x = 0.8 * np.sin(2 * np.pi * rng.uniform(0.01, 0.45, (D, 1)) * n) + 0.05 * rng.standard_normal((D, N))
    xd = torch.from_numpy(x.astype(np.float32)).cuda().repeat((B + D - 1) // D, 1)[:B].contiguous()
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

    def part(title, cols, calls):
        med = {k: [] for k in cols}
        for _ in range(a.rounds):
            for k in cols:
                med[k].append(by_events(calls[k]))
        c = {k: float(np.median(med[k])) for k in cols}
        say(f"{title}: " + "  ".join(f"{k} {c[k]:8.1f}" for k in cols))
        say("          round medians: " + "  ".join(f"{k} {spread(med[k])}" for k in cols))
        return c

    say(f"tools/fold_f32_time.py: B = {B}, filter mode 0xB1, {a.rounds} alternating rounds of {a.calls} timed calls per column; "
        f"us per call, events around the one operation on one stream")
    with SpectrumChain(0) as ch:
        mag = ch.process_f32(xd, out_kind="mag_full")
        mag2 = torch.empty_like(mag)
        rec = {p: ch.spectra_f32(xd, *p) for p in PAIRS}       # the first call allocates the cached workspace
        torch.cuda.synchronize()
        m8 = mag[:256].cpu().numpy()
        for p in PAIRS:                                        # the timed call computes what the mirror says: the first 256 frames
            peak, power, _ = frames.fold_of_mags(m8, *p)
            got = rec[p][:256 // p[0]].cpu().numpy()
            same = np.array_equal(got[..., 0].view(np.uint32), peak.view(np.uint32)) and \
                np.array_equal(got[..., 1].view(np.uint32), power.view(np.uint32))
            say(f"{name(p)}: records of the first 256 frames {'equal' if same else 'DIFFER FROM'} frames.fold_of_mags bit for bit")
        mag_bytes = B * 65536
        say(f"magnitude tensor {mag_bytes >> 20} MiB; result bytes per input frame: mag_full 65536  "
            + "  ".join(f"{name(p)} {131072 // (p[0] * p[1])}" for p in PAIRS))
        # part 1: the fold alone against a device-to-device copy of the same tensor; 1a on rotating inputs, 1b on one
        mags = [mag] + [mag.clone() for _ in range(2)]
        dsts = [mag2, torch.empty_like(mag)]
        turn = itertools.count()
        for tag, srcs in (("1a, rotating inputs", mags), ("1b, one input     ", mags[:1])):
            def copy(srcs=srcs):
                i = next(turn)
                dsts[i % 2].copy_(srcs[i % len(srcs)])

            calls = {"copy_": copy}
            for p in PAIRS:
                calls[f"fold {name(p)}"] = lambda p=p, srcs=srcs: ch.fold_mag_f32(srcs[next(turn) % len(srcs)], *p, out=rec[p])
            c = part(f"part {tag}", list(calls), calls)
            say("          fold / copy_ (bytes moved, fold / copy: " + " ".join(f"{(1 + 2 / (p[0] * p[1])) / 2:.3f}" for p in PAIRS) + "): "
                + "  ".join(f"{name(p)} {c[f'fold {name(p)}'] / c['copy_']:.3f}" for p in PAIRS))
            say("          input bytes / time: copy_ " + f"{mag_bytes / c['copy_'] / 1e6:.2f} TB/s  "
                + "  ".join(f"{name(p)} {mag_bytes / c[f'fold {name(p)}'] / 1e6:.2f} TB/s" for p in PAIRS))
        del mags[1:], dsts[1:]
        # part 2: the composed call against the call it contains
        calls2 = {"mag_full": lambda: ch.process_f32(xd, out=mag, out_kind="mag_full")}
        for p in PAIRS:
            calls2[f"spectra {name(p)}"] = lambda p=p: ch.spectra_f32(xd, *p, out=rec[p])
        cols = list(calls2)
        c2 = part("part 2, on the device", cols, calls2)
        say("          spectra / mag_full: " + "  ".join(f"{name(p)} {c2[f'spectra {name(p)}'] / c2['mag_full']:.3f}" for p in PAIRS)
            + "   spectra - mag_full - fold [us]: "
            + "  ".join(f"{name(p)} {c2[f'spectra {name(p)}'] - c2['mag_full'] - c[f'fold {name(p)}']:+.1f}" for p in PAIRS))
        # part 3: with the result copied to pinned host memory behind each call
        host = torch.empty(mag.numel() * 4, dtype=torch.uint8).pin_memory()

        def with_copy(fn, t):
            src, dst = t.view(-1).view(torch.uint8), host[:t.numel() * t.element_size()]
            return lambda: (fn(), dst.copy_(src, non_blocking=True))

        calls3 = {"mag_full": with_copy(calls2["mag_full"], mag)}
        for p in PAIRS:
            calls3[f"spectra {name(p)}"] = with_copy(calls2[f"spectra {name(p)}"], rec[p])
        c3 = part("part 3, call + copy  ", list(calls3), calls3)
        say("          mag_full / spectra (bound: the byte ratio A W / 2): "
            + "  ".join(f"{name(p)} {c3['mag_full'] / c3[f'spectra {name(p)}']:.2f}" for p in PAIRS))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
