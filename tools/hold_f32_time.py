#!/usr/bin/env python3
"""Cost of the percentile traces (include/specan_hold.h; SpectrumChain.hold_ranks and hold_f32) on B = 4096 rows.  Every column is
timed between a pair of events on the current stream around the one operation; the columns of a part alternate in one process
over several rounds (each round: a warm-up call, then a timed train), and a ratio is read beside the spread of its columns'
own round medians, never against a stored number.
Part 1: the sort alone through the C entry point (no allocation between the events) at (A, q) = (4, 1), (16, 1), (16, 3),
        (128, 1), (128, 3), (128, 8), (15, 1), for field 0 on 256 MiB of magnitudes (4096 rows; 4095 at A = 15) and for field 2
        on 256 MiB of records (2048 rows; 2040 at A = 15), the points exp(uniform +-60), against the yardsticks of the same
        run: a device-to-device copy_ of the same input tensor, and what a caller can do today without the host, torch.sort
        along the frames of [G, A, N] and torch.kthvalue (one rank) of the same points into preallocated outputs.  Every column
        rotates over three equal inputs (768 MiB), so that no call finds its input in the 256 MiB Infinity Cache.  With --lib,
        a second build of the library (csrc/hold_f32.hip with -DSA_HOLD_SELECT: selection per lane instead of the sorting
        network) is timed as the columns "select" in the same rounds.
Part 2: hold_f32 against process_f32('mag_full'), the call it contains.
Part 3: both with the result copied to pinned host memory behind the call, against 'mag_full' + its copy.
usage: hold_f32_time.py [--rounds R] [--calls C] [--batch B] [--lib FILE] [--out FILE]   (GPU; prints its lines, and writes them to
FILE when one is given: profiles/r27_hold_f32.txt holds a run's lines between sections written by hand, so it is no default)"""
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
SHAPES = ((4, 1), (16, 1), (16, 3), (128, 1), (128, 3), (128, 8), (15, 1))


def spread(v):
    return f"{min(v):.1f}-{max(v):.1f} ({max(v) / min(v):.3f})"


def ranks_of(A, q):
    """q ranks across a group of A, the lower median first"""
    return [(A - 1) // 2, 0, A - 1, A // 4, (3 * A) // 4, A // 8, (7 * A) // 8, A // 3][:q]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--lib", default=None)
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

    say(f"tools/hold_f32_time.py: B = {B}, {a.rounds} alternating rounds of {a.calls} timed calls per column; us per call, events "
        f"around the one operation on one stream")
    libs = {"hold": abi.hold_lib()}
    if a.lib is not None:
        other = ctypes.CDLL(os.path.abspath(a.lib))                # torch is imported: it binds to the runtime torch mapped
        for name, (restype, argtypes) in abi.HOLD_SIGNATURES.items():
            getattr(other, name).restype, getattr(other, name).argtypes = restype, argtypes
        libs["select"] = other
    stream = torch.cuda.current_stream().cuda_stream
    with SpectrumChain(0) as ch:
        # part 1: the sort alone against the yardsticks, inputs rotating over three tensors
        turn = itertools.count()
        g = torch.Generator(device="cuda").manual_seed(11)
        for field in (0, 2):
            rows = B if field == 0 else B // 2
            t = torch.exp(torch.empty((rows, N) if field == 0 else (rows, N, 2), dtype=torch.float32,
                                      device="cuda").uniform_(-60.0, 60.0, generator=g))
            srcs = [t] + [t.clone() for _ in range(2)]
            dst = torch.empty_like(t)
            out = torch.empty((rows // 4 * 8 * N,), dtype=torch.float32, device="cuda")       # the largest output: A = 4, and 8 ranks
            torch.cuda.synchronize()
            for A, q in SHAPES:
                R = rows // A * A
                G = R // A
                ranks = ranks_of(A, q)
                c_ranks = (ctypes.c_int32 * q)(*ranks)
                name = "power" if field else None
                head = np.ascontiguousarray(t[:2 * A].cpu().numpy())
                want = frames.holds_of_rows(head, ranks, A, field=name).view(np.uint32)
                for k, L in libs.items():                      # the timed call computes what the mirror says
                    rc = L.sa_hold_f32(t.data_ptr(), field, out.data_ptr(), 2 * A, A, q, c_ranks, stream)
                    assert rc == 0, L.sa_hold_last_error()
                    same = np.array_equal(out[:2 * q * N].cpu().numpy().view(np.uint32).reshape(2, q, N), want)
                    say(f"field {field}, A {A}, q {q}, {k}: the first 2 groups {'equal' if same else 'DIFFER FROM'} frames.holds_of_rows "
                        f"bit for bit")
                # the points as torch sees them: [G, A, N], strided in records
                pts = [(s[:R] if field == 0 else s[:R, :, 1]).unflatten(0, (G, A)) for s in srcs]
                s_val = torch.empty((G, A, N), dtype=torch.float32, device="cuda")
                s_idx = torch.empty((G, A, N), dtype=torch.int64, device="cuda")
                k_val = torch.empty((G, N), dtype=torch.float32, device="cuda")
                k_idx = torch.empty((G, N), dtype=torch.int64, device="cuda")

                def copy():
                    dst.copy_(srcs[next(turn) % 3])

                def sort():
                    torch.sort(pts[next(turn) % 3], dim=1, out=(s_val, s_idx))

                def kth():
                    torch.kthvalue(pts[next(turn) % 3], ranks[0] + 1, dim=1, out=(k_val, k_idx))

                def hold(L):
                    rc = L.sa_hold_f32(srcs[next(turn) % 3].data_ptr(), field, out.data_ptr(), R, A, q, c_ranks, stream)
                    assert rc == 0, L.sa_hold_last_error()

                calls = {"copy_": copy, "sort": sort, "kthvalue": kth}
                for k, L in libs.items():
                    calls[k] = lambda L=L: hold(L)
                c = part(f"part 1, field {field}, A {A:3d}, q {q}, {R} rows", list(calls), calls)
                say("          " + "  ".join(f"{k} / copy_ {c[k] / c['copy_']:.3f}  sort / {k} {c['sort'] / c[k]:.1f}  kthvalue / {k} "
                                            f"{c['kthvalue'] / c[k]:.1f}  input bytes / time {R * N * 4 * (2 if field else 1) / c[k] / 1e6:.2f} "
                                            f"TB/s" for k in libs)
                    + f"   copy_ {t.numel() * 4 / c['copy_'] / 1e6:.2f} TB/s")
                del pts, s_val, s_idx, k_val, k_idx
            del srcs, dst, out, t
            torch.cuda.empty_cache()
        # part 2: the composed call against the call it contains
        ch.set_filter_mode(0xB1)
        rng = np.random.default_rng(7)
        n = np.arange(N)
        D = min(B, 256)                                        # three tones + noise: 256 distinct frames, repeated
        x = sum(amp * np.sin(2 * np.pi * rng.uniform(0.01, 0.45, (D, 1)) * n) for amp in (0.5, 0.2, 0.08)) + 0.05 * rng.standard_normal((D, N))
        xd = torch.from_numpy(x.astype(np.float32)).cuda().repeat((B + D - 1) // D, 1)[:B].contiguous()
        mag = ch.process_f32(xd, out_kind="mag_full")
        kw = {"A 16 q 0.5": dict(q=0.5, group=16), "A 16 q 3": dict(q=[0.1, 0.5, 0.9], group=16), "A 128 q 0.5": dict(q=0.5, group=128),
              "A 128 q 3": dict(q=[0.1, 0.5, 0.9], group=128)}
        outs = {name: torch.empty((B // v["group"], len(v["q"]) if isinstance(v["q"], list) else 1, N), dtype=torch.float32, device="cuda")
                for name, v in kw.items()}
        calls2 = {"mag_full": lambda: ch.process_f32(xd, out=mag, out_kind="mag_full")}
        for name, v in kw.items():
            calls2[name] = lambda name=name, v=v: ch.hold_f32(xd, out=outs[name], **v)
        c2 = part("part 2, on the device", list(calls2), calls2)
        say("          hold_f32 / mag_full: " + "  ".join(f"{k} {c2[k] / c2['mag_full']:.3f}" for k in kw))
        # part 3: with the result copied to pinned host memory behind each call
        host = torch.empty(mag.numel() * 4, dtype=torch.uint8).pin_memory()

        def mag_and_copy():
            calls2["mag_full"]()
            host.copy_(mag.view(-1).view(torch.uint8), non_blocking=True)

        def hold_and_copy(name):
            calls2[name]()
            o = outs[name]
            host[:o.numel() * 4].copy_(o.view(-1).view(torch.uint8), non_blocking=True)

        calls3 = {"mag_full": mag_and_copy}
        for name in kw:
            calls3[name] = lambda name=name: hold_and_copy(name)
        c3 = part("part 3, call + copy  ", list(calls3), calls3)
        say("          mag_full / hold_f32: " + "  ".join(f"{k} {c3['mag_full'] / c3[k]:.2f}" for k in kw))
    if a.out is not None:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
