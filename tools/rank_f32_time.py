#!/usr/bin/env python3
"""Cost of the order statistics (include/specan_rank.h; SpectrumChain.order_stats and noise_floor_f32) on B = 4096 rows.  Every
column is timed between a pair of events on the current stream around the one operation; the columns of a part alternate in
one process over several rounds (each round: a warm-up call, then a timed train), and a ratio is read beside the spread of
its columns' own round medians, never against a stored number.
Part 1: the selection alone through the C entry point (no allocation between the events), q = 1, 3, 8, for field 0 on 256 MiB
        of magnitudes (4096 rows) and for field 2 on 256 MiB of records (2048 rows), on three data sets -- "tones": three tones
        plus noise through filter mode 0xB1 ('mag_full', and the records of spectra_f32(group=2)); "wide": exp(uniform +-60);
        "const": one value -- against the two yardsticks of the same run: a device-to-device copy_ of the same input tensor,
        and what a caller can do today without the host, torch.sort and torch.kthvalue (one rank) of the same points into
        preallocated outputs.  Every column rotates over three equal inputs (768 MiB), so that no call finds its input in the
        256 MiB Infinity Cache.
Part 2: noise_floor_f32 against process_f32('mag_full'), the call it contains; and with group=4.
Part 3: both with the result copied to pinned host memory behind the call, against 'mag_full' + its copy.
usage: rank_f32_time.py [--rounds R] [--calls C] [--batch B] [--out FILE]   (GPU; prints its lines, and writes them to FILE when one
is given: profiles/r18_rank_f32.txt holds a run's lines between sections written by hand, so it is no default)"""
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
RANKS = {"q1": [8191], "q3": [1638, 8191, 14744], "q8": [0, 1638, 4095, 8191, 12287, 14744, 16220, 16383]}


def spread(v):
    return f"{min(v):.1f}-{max(v):.1f} ({max(v) / min(v):.3f})"


def main():
    ap = argparse.ArgumentParser()
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

    say(f"tools/rank_f32_time.py: B = {B}, {a.rounds} alternating rounds of {a.calls} timed calls per column; us per call, events "
        f"around the one operation on one stream")
    L = abi.rank_lib()
    stream = torch.cuda.current_stream().cuda_stream
    c_ranks = {k: (ctypes.c_int32 * len(v))(*v) for k, v in RANKS.items()}
    with SpectrumChain(0) as ch:
        ch.set_filter_mode(0xB1)
        mag = ch.process_f32(xd, out_kind="mag_full")
        torch.cuda.synchronize()

        def data_set(name, field):
            """256 MiB of the data set in the layout: float32 [B, N], or records [B / 2, N, 2] whose second float is the point"""
            if name == "tones":
                return mag.clone() if field == 0 else ch.spectra_f32(xd, 2)
            g = torch.Generator(device="cuda").manual_seed(11)
            shape = (B, N) if field == 0 else (B // 2, N, 2)
            if name == "wide":
                return torch.exp(torch.empty(shape, dtype=torch.float32, device="cuda").uniform_(-60.0, 60.0, generator=g))
            return torch.full(shape, 0.37, dtype=torch.float32, device="cuda")

        # part 1: the selection alone against the two yardsticks, inputs rotating over three tensors
        turn = itertools.count()
        out = torch.empty((B, 8), dtype=torch.float32, device="cuda")
        for name in ("tones", "wide", "const"):
            for field in (0, 2):
                t = data_set(name, field)
                torch.cuda.synchronize()
                R = t.shape[0]
                head = np.ascontiguousarray(t[:64].cpu().numpy())
                for k, ranks in RANKS.items():                 # the timed call computes what the mirror says
                    got = ch.order_stats(t[:64], ranks, field="power" if field else None)
                    want = frames.ranks_of_rows(head, ranks, field="power" if field else None)
                    same = np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
                    say(f"{name}, field {field}, {k}: the first 64 rows {'equal' if same else 'DIFFER FROM'} frames.ranks_of_rows bit for bit")
                srcs = [t] + [t.clone() for _ in range(2)]
                dst = torch.empty_like(t)
                pts = [s if field == 0 else s[..., 1] for s in srcs]              # the points as torch sees them (strided in records)
                s_val = torch.empty((R, N), dtype=torch.float32, device="cuda")
                s_idx = torch.empty((R, N), dtype=torch.int64, device="cuda")
                k_val = torch.empty((R,), dtype=torch.float32, device="cuda")
                k_idx = torch.empty((R,), dtype=torch.int64, device="cuda")

                def copy():
                    dst.copy_(srcs[next(turn) % 3])

                def sort():
                    torch.sort(pts[next(turn) % 3], dim=1, out=(s_val, s_idx))

                def kth():
                    torch.kthvalue(pts[next(turn) % 3], 8192, dim=1, out=(k_val, k_idx))

                def rank(k):
                    rc = L.sa_rank_f32(srcs[next(turn) % 3].data_ptr(), field, out.data_ptr(), R, len(RANKS[k]), c_ranks[k], 0, N, stream)
                    assert rc == 0, L.sa_rank_last_error()

                calls = {"copy_": copy, "sort": sort, "kthvalue": kth}
                for k in RANKS:
                    calls[k] = lambda k=k: rank(k)
                c = part(f"part 1, {name}, field {field}, {R} rows", list(calls), calls)
                say("          rank / copy_: " + "  ".join(f"{k} {c[k] / c['copy_']:.3f}" for k in RANKS)
                    + "   sort / rank: " + "  ".join(f"{k} {c['sort'] / c[k]:.1f}" for k in RANKS)
                    + "   kthvalue / rank: " + "  ".join(f"{k} {c['kthvalue'] / c[k]:.1f}" for k in RANKS)
                    + f"   input bytes / time: copy_ {t.numel() * 4 / c['copy_'] / 1e6:.2f} TB/s  "
                    + "  ".join(f"{k} {t.numel() * 4 / c[k] / 1e6:.2f}" for k in RANKS))
                del srcs, dst, pts, s_val, s_idx, k_val, k_idx, t
                torch.cuda.empty_cache()
        # part 2: the composed call against the call it contains
        kw = {"q 0.5": dict(q=0.5), "q 3": dict(q=[0.1, 0.5, 0.9]), "q 8": dict(q=[0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99, 1.0]),
              "q 0.5 group4": dict(q=0.5, group=4)}
        outs = {name: torch.empty((B // v.get("group", 1), len(v["q"]) if isinstance(v["q"], list) else 1), dtype=torch.float32, device="cuda")
                for name, v in kw.items()}
        calls2 = {"mag_full": lambda: ch.process_f32(xd, out=mag, out_kind="mag_full")}
        for name, v in kw.items():
            calls2[name] = lambda name=name, v=v: ch.noise_floor_f32(xd, out=outs[name], **v)
        c2 = part("part 2, on the device", list(calls2), calls2)
        say("          noise_floor / mag_full: " + "  ".join(f"{k} {c2[k] / c2['mag_full']:.3f}" for k in kw))
        # part 3: with the result copied to pinned host memory behind each call
        host = torch.empty(mag.numel() * 4, dtype=torch.uint8).pin_memory()

        def mag_and_copy():
            calls2["mag_full"]()
            host.copy_(mag.view(-1).view(torch.uint8), non_blocking=True)

        def floor_and_copy(name):
            calls2[name]()
            o = outs[name]
            host[:o.numel() * 4].copy_(o.view(-1).view(torch.uint8), non_blocking=True)

        calls3 = {"mag_full": mag_and_copy}
        for name in kw:
            calls3[name] = lambda name=name: floor_and_copy(name)
        c3 = part("part 3, call + copy  ", list(calls3), calls3)
        say("          mag_full / noise_floor: " + "  ".join(f"{k} {c3['mag_full'] / c3[k]:.2f}" for k in kw))
    if a.out is not None:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
