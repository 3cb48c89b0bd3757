#!/usr/bin/env python3
"""Cost of the signal list (include/specan_signals.h; SpectrumChain.find_signals and signals_f32) on B = 4096 rows.
Every column is timed between a pair of events on the current stream around the one operation; the columns of a part
alternate in one process over several rounds (each round: a warm-up call, then a timed train), and a ratio is read beside the
spread of its columns' own round medians, never against a stored number.
Part 1: the call alone through the C entry point (no allocation between the events), a threshold per row in device memory,
        at (k, gap, min_width) = (16, 0, 1), (16, 8, 2) and (32, 8, 2) -- for field 0 on 256 MiB of magnitudes (4096 rows) and
        for field 2 on 256 MiB of records (2048 rows), on three data sets -- "noise": |N(0,1)| alone under 6 times each row's
        median, which leaves a handful of on bins in a row at most (counted here); "planted": sixteen emissions of the widths
        1..400 over that noise, 1000 bins apart; "alt": every other bin on, 8192 segments a row -- and on "spread", the
        emissions of "planted" moved so that the tiles they start in belong to the four waves in turn -- against the two
        yardsticks of the same run, a device-to-device copy_ of the same input tensor and the sa_peaks_f32 call with k = 8 on
        the same input, and against what a caller can do today in torch on the same tensors: the on-mask, its differences, and
        nonzero of the starts and of the stops, which brings every segment's bounds to the host's knowledge (a sync) and gives
        neither power nor peak.
        Every column rotates over three equal inputs (768 MiB), so that no call finds its input in the 256 MiB Infinity Cache.
Part 2: signals_f32 with factor = 6 against process_f32('mag_full'), the call it contains; and with group=4.
Part 3: both with the records and counts copied to pinned host memory behind the call, against 'mag_full' + its copy.
usage: signals_cost.py [--rounds R] [--calls C] [--batch B] [--out FILE]   (GPU; prints its lines, and writes them to FILE when
one is given: profiles/r25_signals_f32.txt holds a run's lines between sections written by hand, so it is no default)"""
import argparse
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
CONFIGS = {"k16": (16, 0, 1), "k16g8": (16, 8, 2), "k32g8": (32, 8, 2)}    # name -> (k, gap, min_width)
WIDTHS = (1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 200, 256, 300, 350, 400)  # the planted emissions, 1000 bins apart
FACTOR = 6.0


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

    say(f"tools/signals_cost.py: B = {B}, {a.rounds} alternating rounds of {a.calls} timed calls per column; us per call, events "
        f"around the one operation on one stream")
    L, LP = abi.signals_lib(), abi.peaks_lib()
    stream = torch.cuda.current_stream().cuda_stream
    D = min(B, 256)                                            # 256 distinct rows, repeated
    g = torch.Generator(device="cuda").manual_seed(25)
    noise = torch.randn((D, N), device="cuda", generator=g).abs()
    planted = noise.clone()
    for j, w in enumerate(WIDTHS):
        amp = 8.0 + 8.0 * torch.rand((D, w), device="cuda", generator=g)
        planted[:, 300 + 1000 * j:300 + 1000 * j + w] = amp
    spread_out = noise.clone()                                 # the widest first; slot s starts in tile 4 s + (s & 3): wave s & 3
    for s, (j, w) in enumerate(reversed(list(enumerate(WIDTHS)))):
        a0 = 1024 * s + 256 * (s & 3) + (4 if s & 3 == 3 else 20)
        spread_out[:, a0:a0 + w] = planted[:, 300 + 1000 * j:300 + 1000 * j + w]
    alt = torch.zeros((D, N), device="cuda")
    alt[:, 0::2] = 1.0 + torch.rand((D, N // 2), device="cuda", generator=g)
    sets = {"noise": noise, "planted": planted, "alt": alt, "spread": spread_out}
    n = np.arange(N)
    rng = np.random.default_rng(7)
    x = sum(amp * np.sin(2 * np.pi * rng.uniform(0.01, 0.45, (D, 1)) * n) for amp in (0.5, 0.2, 0.08)) + 0.05 * rng.standard_normal((D, N))
    xd = torch.from_numpy(x.astype(np.float32)).cuda().repeat((B + D - 1) // D, 1)[:B].contiguous()
    with SpectrumChain(0) as ch:
        def data_set(name, field):
            """256 MiB of the data set in the layout: float32 [B, N], or records [B / 2, N, 2] whose second float is the point"""
            R = B if field == 0 else B // 2
            rows = sets[name].repeat((R + D - 1) // D, 1)[:R].contiguous()
            if field == 0:
                return rows
            rec = torch.zeros((R, N, 2), dtype=torch.float32, device="cuda")
            rec[..., 1] = rows
            return rec

        def threshold(name, t, fname):
            """a threshold per row: 6 times the row's median, or 0.5 for the alternating row (whose median is no noise floor)"""
            if name == "alt":
                return torch.full((t.shape[0],), 0.5, dtype=torch.float32, device="cuda")
            return ch.order_stats(t, [frames.rank_of_quantile(0.5, N)], field=fname)[:, 0] * FACTOR

        # part 1: the call alone against the yardsticks, inputs rotating over three tensors
        turn = itertools.count()
        for name in sets:
            for field in (0, 2):
                t = data_set(name, field)
                R = t.shape[0]
                fname = "power" if field else None
                thr = threshold(name, t, fname)
                torch.cuda.synchronize()
                head, thr_head = np.ascontiguousarray(t[:64].cpu().numpy()), thr[:64].cpu().numpy()
                for c, (k, gap, mw) in CONFIGS.items():          # the timed call computes what the mirror says
                    got = ch.find_signals(t[:64], k, thr[:64], gap=gap, min_width=mw, field=fname)
                    want = frames.signals_of_rows(head, k=k, threshold=thr_head, gap=gap, min_width=mw, field=fname)
                    rec = torch.cat([got[0], got[1].view(torch.int32)[..., None], got[2][..., None]], -1).cpu().numpy()
                    ref = np.stack([want[0]["start"], want[0]["stop"], want[0]["peak"].view(np.int32), want[0]["peak_bin"]], -1)
                    same = (np.array_equal(rec, ref) and np.array_equal(got[3].cpu().numpy().view(np.int64), want[0]["power"].view(np.int64))
                            and np.array_equal(got[4].cpu().numpy(), want[1]))
                    st = want[1]
                    say(f"{name}, field {field}, {c}: the first 64 rows {'equal' if same else 'DIFFER FROM'} frames.signals_of_rows bit "
                        f"for bit; kept segments per row {st[:, 0].min()}..{st[:, 0].max()}, on bins {st[:, 1].min()}..{st[:, 1].max()}, "
                        f"covered {st[:, 2].min()}..{st[:, 2].max()}")
                if name == "noise":
                    on = ch.find_signals(t, 1, thr, field=fname)[4][:, 1]
                    say(f"noise, field {field}: on bins per row over all {R} rows: min {int(on.min())}, median {int(on.median())}, "
                        f"max {int(on.max())}, mean {float(on.float().mean()):.2f}")
                srcs = [t] + [t.clone() for _ in range(2)]
                dst = torch.empty_like(t)
                out = torch.empty((R, 32, 6), dtype=torch.int32, device="cuda")
                stats = torch.empty((R, 3), dtype=torch.int32, device="cuda")
                peaks_out = torch.empty((R, 8, 2), dtype=torch.int32, device="cuda")
                peaks_count = torch.empty((R,), dtype=torch.int32, device="cuda")

                def copy():
                    dst.copy_(srcs[next(turn) % 3])

                def peaks8():
                    rc = LP.sa_peaks_f32(srcs[next(turn) % 3].data_ptr(), field, peaks_out.data_ptr(), peaks_count.data_ptr(), R, 8, 0.0, 0, N,
                                         1, stream)
                    assert rc == 0, LP.sa_peaks_last_error()

                def torch_bounds():
                    """gap 0, min_width 1, in torch: the on-mask, its differences, the starts and the stops on the host's side"""
                    src = srcs[next(turn) % 3]
                    v = (src if field == 0 else src[..., 1]).abs()
                    on = (v >= thr[:, None]) & (v > 0)
                    d = torch.diff(on.to(torch.int8), dim=1, prepend=on.new_zeros((R, 1), dtype=torch.int8),
                                   append=on.new_zeros((R, 1), dtype=torch.int8))
                    return torch.nonzero(d == 1), torch.nonzero(d == -1), on.sum(1)

                def call(c):
                    k, gap, mw = CONFIGS[c]
                    rc = L.sa_signals_f32(srcs[next(turn) % 3].data_ptr(), field, thr.data_ptr(), 0.0, out.data_ptr(), stats.data_ptr(), R, k,
                                          0, N, gap, mw, stream)
                    assert rc == 0, L.sa_signals_last_error()

                calls = {"copy_": copy, "peaks8": peaks8, "torch": torch_bounds}
                for c in CONFIGS:
                    calls[c] = lambda c=c: call(c)
                m = part(f"part 1, {name}, field {field}, {R} rows", list(calls), calls)
                say("          signals / copy_: " + "  ".join(f"{c} {m[c] / m['copy_']:.3f}" for c in CONFIGS)
                    + f"   peaks8 / copy_: {m['peaks8'] / m['copy_']:.3f}"
                    + "   signals / peaks8: " + "  ".join(f"{c} {m[c] / m['peaks8']:.3f}" for c in CONFIGS)
                    + f"   torch / k16: {m['torch'] / m['k16']:.1f}"
                    + f"   input bytes / time: copy_ {t.numel() * 4 / m['copy_'] / 1e6:.2f} TB/s  "
                    + "  ".join(f"{c} {t.numel() * 4 / m[c] / 1e6:.2f}" for c in CONFIGS))
                del srcs, dst, t
                torch.cuda.empty_cache()
        # part 2: the composed call against the call it contains
        ch.set_filter_mode(0xB1)
        mag = ch.process_f32(xd, out_kind="mag_full")
        torch.cuda.synchronize()
        kw = {"k16": dict(k=16), "k16g8": dict(k=16, gap=8, min_width=2), "k32g8": dict(k=32, gap=8, min_width=2),
              "k16 group4": dict(k=16, group=4)}
        outs = {name: (torch.empty((B // v.get("group", 1), v["k"], 6), dtype=torch.int32, device="cuda"),
                       torch.empty((B // v.get("group", 1), 3), dtype=torch.int32, device="cuda")) for name, v in kw.items()}
        calls2 = {"mag_full": lambda: ch.process_f32(xd, out=mag, out_kind="mag_full")}
        for name, v in kw.items():
            calls2[name] = lambda name=name, v=v: ch.signals_f32(xd, factor=FACTOR, out=outs[name][0], stats=outs[name][1], **v)
        st = ch.signals_f32(xd, 16, factor=FACTOR)[4]
        say(f"part 2: three tones plus noise through filter mode 0xB1, factor {FACTOR}: kept segments per row "
            f"{int(st[:, 0].min())}..{int(st[:, 0].max())}, on bins {int(st[:, 1].min())}..{int(st[:, 1].max())}")
        c2 = part("part 2, on the device", list(calls2), calls2)
        say("          signals_f32 / mag_full: " + "  ".join(f"{k} {c2[k] / c2['mag_full']:.3f}" for k in kw))
        # part 3: with the result copied to pinned host memory behind each call
        host = torch.empty(mag.numel() * 4, dtype=torch.uint8).pin_memory()

        def mag_and_copy():
            calls2["mag_full"]()
            host.copy_(mag.view(-1).view(torch.uint8), non_blocking=True)

        def signals_and_copy(name):
            calls2[name]()
            o, s = outs[name]
            host[:o.numel() * 4].copy_(o.view(-1).view(torch.uint8), non_blocking=True)
            host[o.numel() * 4:(o.numel() + s.numel()) * 4].copy_(s.view(-1).view(torch.uint8), non_blocking=True)

        calls3 = {"mag_full": mag_and_copy}
        for name in kw:
            calls3[name] = lambda name=name: signals_and_copy(name)
        c3 = part("part 3, call + copy  ", list(calls3), calls3)
        say("          mag_full / signals_f32: " + "  ".join(f"{k} {c3['mag_full'] / c3[k]:.2f}" for k in kw))
    if a.out is not None:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
