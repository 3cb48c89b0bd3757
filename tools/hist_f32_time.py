#!/usr/bin/env python3
"""Cost of the level histogram (include/specan_hist.h; SpectrumChain.level_hist and persistence_f32) on B = 4096 rows.  Every
column is timed between a pair of events on the current stream around the one operation; the columns of a part alternate in
one process over several rounds (each round: a warm-up call, then a timed train), and a ratio is read beside the spread of
its columns' own round medians, never against a stored number.
Part 1: the count alone through the C entry point (no allocation between the events) at (A, W, L) = (4096, 16, 64),
        (256, 16, 64), (16, 1, 64) and (4096, 64, 16) on 256 MiB of magnitudes, on three data sets -- "tones": three tones plus
        noise through filter mode 0xB1 ('mag_full'); "wide": exp(uniform +-60); "const": one value, the worst case for adds
        to one LDS word -- against the two yardsticks of the same run: a device-to-device copy_ of the same input tensor, and
        what a caller can do today without the host, torch.bucketize(mag, edges, right=True) plus the cell's base, then
        scatter_add_ of ones into a zeroed [G, C, L] (and torch.bincount of the same cells), into preallocated tensors where
        the operation takes one.  Every column rotates over three equal inputs (768 MiB), so that no call finds its input in
        the 256 MiB Infinity Cache.  The torch columns are slow and run a quarter of the calls.
Part 2: persistence_f32 against process_f32('mag_full'), the call it contains.
Part 3: the same with the result copied to pinned host memory behind the call, against 'mag_full' + its copy.
usage: hist_f32_time.py [--part 1|2|3] [--data tones|wide|const] [--rounds R] [--calls C] [--batch B] [--out FILE]   (GPU; one
part, and in part 1 one data set, per process, so that each can run under a time limit of its own; prints its lines and appends
them to FILE when one is given: profiles/r19_hist_f32.txt holds a run's lines between sections written by hand, so it is no
default)"""
import argparse
import ctypes
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fpga_real_time_fft_analyzer_amd import abi, frames  # noqa: E402
from fpga_real_time_fft_analyzer_amd.chain import SpectrumChain  # noqa: E402

N = 16384
SHAPES = ((4096, 16, 64), (256, 16, 64), (16, 1, 64), (4096, 64, 16))     # (A, W, L)


def spread(v):
    return f"{min(v):.1f}-{max(v):.1f} ({max(v) / min(v):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", type=int, default=1, choices=(1, 2, 3))
    ap.add_argument("--data", default="tones", choices=("tones", "wide", "const"))
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--calls", type=int, default=16)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    B = a.batch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(7)
    n = np.arange(N)
    D = min(B, 256)                                            # three tones + noise: 256 distinct frames, repeated
    x = sum(amp * np.sin(2 * np.pi * rng.uniform(0.01, 0.45, (D, 1)) * n) for amp in (0.5, 0.2, 0.08)) + 0.05 * rng.standard_normal((D, N))
    xd = torch.from_numpy(x.astype(np.float32)).cuda().repeat((B + D - 1) // D, 1)[:B].contiguous()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]

    def by_events(fn, calls):
        """median us of `fn` over a train of `calls`, each between its own pair of events on the current stream"""
        fn()
        torch.cuda.synchronize()
        for s, e in ev[:calls]:
            s.record()
            fn()
            e.record()
        torch.cuda.synchronize()
        return float(np.median([s.elapsed_time(e) for s, e in ev[:calls]])) * 1e3

    def part(title, cols, calls, slow=()):
        med = {k: [] for k in cols}
        for _ in range(a.rounds):
            for k in cols:
                med[k].append(by_events(calls[k], max(a.calls // 4, 1) if k in slow else a.calls))
        c = {k: float(np.median(med[k])) for k in cols}
        say(f"{title}: " + "  ".join(f"{k} {c[k]:8.1f}" for k in cols))
        say("          round medians: " + "  ".join(f"{k} {spread(med[k])}" for k in cols))
        return c

    say(f"tools/hist_f32_time.py --part {a.part}" + (f" --data {a.data}" if a.part == 1 else "") + f": B = {B}, {a.rounds} alternating "
        f"rounds of {a.calls} timed calls per column; us per call, events around the one operation on one stream")
    L = abi.hist_lib()
    stream = torch.cuda.current_stream().cuda_stream
    with SpectrumChain(0) as ch:
        ch.set_filter_mode(0xB1)
        mag = ch.process_f32(xd, out_kind="mag_full")
        torch.cuda.synchronize()
        top = float(mag.max().item())
        if a.part == 1:
            name = a.data
            if name == "tones":
                t = mag.clone()
            elif name == "wide":
                g = torch.Generator(device="cuda").manual_seed(11)
                t = torch.exp(torch.empty((B, N), dtype=torch.float32, device="cuda").uniform_(-60.0, 60.0, generator=g))
            else:
                t = torch.full((B, N), 0.37, dtype=torch.float32, device="cuda")
            srcs = [t] + [t.clone() for _ in range(2)]
            dst = torch.empty_like(t)
            ones = torch.ones((B * N,), dtype=torch.int32, device="cuda")
            rows = torch.arange(B, device="cuda").view(B, 1)
            bins = torch.arange(N, device="cuda").view(1, N)
            turn = itertools.count()
            for A, W, nlev in SHAPES:
                A = min(A, B)
                G, cols = B // A, N // W
                if name == "tones":
                    edges = frames.level_edges_db(top, 100.0, nlev)
                elif name == "wide":
                    edges = np.exp(np.linspace(-55.0, 55.0, nlev - 1)).astype(np.float32)
                else:
                    edges = frames.level_edges_db(1.0, 60.0, nlev)
                c_edges = (ctypes.c_float * (nlev - 1))(*edges)
                edges_t = torch.from_numpy(edges).cuda()
                out = torch.empty((G, cols, nlev), dtype=torch.uint32, device="cuda")
                acc = torch.empty((G * cols * nlev,), dtype=torch.int32, device="cuda")
                base = ((rows // A) * cols + bins // W) * nlev                    # int64 [B, N]: the cell of level 0
                level = torch.empty((B, N), dtype=torch.int64, device="cuda")

                def copy():
                    dst.copy_(srcs[next(turn) % 3])

                def hist():
                    rc = L.sa_hist_f32(srcs[next(turn) % 3].data_ptr(), out.data_ptr(), B, A, W.bit_length() - 1, nlev, c_edges, 0, N, stream)
                    assert rc == 0, L.sa_hist_last_error()

                def cells():
                    torch.bucketize(srcs[next(turn) % 3], edges_t, right=True, out=level)
                    return level.add_(base).view(-1)

                def scatter():
                    acc.zero_()
                    acc.scatter_add_(0, cells(), ones)

                def bincount():
                    return torch.bincount(cells(), minlength=G * cols * nlev)

                # the timed calls compute the same counters: the kernel, the mirror on the first group, and the torch forms
                hist()
                scatter()
                same = torch.equal(out.view(torch.int32).view(-1), acc) and torch.equal(bincount().to(torch.int32), acc)
                head = frames.hist_of_rows(t[:min(A, 64)].cpu().numpy(), edges, group=min(A, 64), bucket=W)
                first = ch.level_hist(t[:min(A, 64)], edges, bucket=W).cpu().numpy()
                say(f"{name}, A {A}, W {W}, L {nlev}: the call {'equals' if same else 'DIFFERS FROM'} bucketize + scatter_add_ and bincount on all "
                    f"{G * cols * nlev} counters; {min(A, 64)} rows {'equal' if np.array_equal(head, first) else 'DIFFER FROM'} frames.hist_of_rows; "
                    f"fullest level holds {int(acc.view(G, cols, nlev).sum(dim=(0, 1)).max().item()) / (B * N):.3f} of the points")
                calls = {"copy_": copy, "hist": hist, "scatter_add_": scatter, "bincount": bincount}
                c = part(f"part 1, {name}, A {A}, W {W}, L {nlev}", list(calls), calls, slow=("scatter_add_", "bincount"))
                say(f"          hist / copy_: {c['hist'] / c['copy_']:.3f}   scatter_add_ / hist: {c['scatter_add_'] / c['hist']:.1f}   "
                    f"bincount / hist: {c['bincount'] / c['hist']:.1f}   input bytes / time: copy_ {t.numel() * 4 / c['copy_'] / 1e6:.2f} TB/s  "
                    f"hist {t.numel() * 4 / c['hist'] / 1e6:.2f}   bytes written by hist: {out.numel() * 4}")
                del out, acc, base, level
                torch.cuda.empty_cache()
        else:
            edges = frames.level_edges_db(top, 100.0, 64)
            kw = {"A 4096 W 16": dict(bucket=16), "A 256 W 16": dict(group=min(256, B), bucket=16), "A 16 W 1": dict(group=16, bucket=1),
                  "A 4096 W 64 L 16": dict(bucket=64, edges=frames.level_edges_db(top, 100.0, 16))}
            outs = {k: torch.empty((B // v.get("group", B), N // v["bucket"], len(v.get("edges", edges)) + 1), dtype=torch.uint32, device="cuda")
                    for k, v in kw.items()}

            def mag_full():
                ch.process_f32(xd, out=mag, out_kind="mag_full")

            def persistence(k):
                ch.persistence_f32(xd, **dict(dict(edges=edges, out=outs[k]), **kw[k]))

            if a.part == 2:
                calls2 = {"mag_full": mag_full}
                for k in kw:
                    calls2[k] = lambda k=k: persistence(k)
                c2 = part("part 2, on the device", list(calls2), calls2)
                say("          persistence / mag_full: " + "  ".join(f"{k} {c2[k] / c2['mag_full']:.3f}" for k in kw))
            else:
                host = torch.empty(max(mag.numel(), max(o.numel() for o in outs.values())) * 4, dtype=torch.uint8).pin_memory()

                def mag_and_copy():
                    mag_full()
                    host[:mag.numel() * 4].copy_(mag.view(-1).view(torch.uint8), non_blocking=True)

                def persistence_and_copy(k):
                    persistence(k)
                    o = outs[k]
                    host[:o.numel() * 4].copy_(o.view(-1).view(torch.uint8), non_blocking=True)

                calls3 = {"mag_full": mag_and_copy}
                for k in kw:
                    calls3[k] = lambda k=k: persistence_and_copy(k)
                c3 = part("part 3, call + copy  ", list(calls3), calls3)
                say("          mag_full / persistence: " + "  ".join(f"{k} {c3['mag_full'] / c3[k]:.2f}" for k in kw)
                    + "   result bytes: " + "  ".join(f"{k} {outs[k].numel() * 4}" for k in kw))
    if a.out is not None:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
