#!/usr/bin/env python3
"""Diagnostic: the integer chain's three output kinds (iq, mag, marker) at B = 4096 in filter modes 0xB1, 0x00 and 0xA2,
in one process, plus the route a caller had before the marker output existed: process_q15 followed by the decode and
max / argmax as torch ops on the device.

  - device time per call from the launch-timing ring (sa_set_profiling): cascade + FFT of one call, events riding on
    the dispatch packets.  The kinds alternate round by round over 4 rotating buffer pairs (one pair would sit in the
    Infinity Cache from launch to launch); per kind the median over all timed calls and the spread of the round medians.
  - wall time per call of a stream-ordered train ending in a synchronise, for the three kinds and the torch route: the
    only clock that sees the torch kernels too.  `marker` against `iq+torch` is the ratio a caller gains.
  - with a second library (a build of another commit: `make -C fpga_real_time_fft_analyzer_amd/csrc ab NAME=parent` in a
    checkout of it, the .so copied next to the package's): its sa_process_q15 against this tree's "iq" kind, same
    handle settings, interleaved in the same rounds, device time from each library's own ring.

usage: q15_out_kinds.py [--rounds R] [--calls C] [--ab libspecan_ab_parent.so] [--batch B]   (GPU)"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fpga_real_time_fft_analyzer_amd.chain import SpectrumChain  # noqa: E402

KINDS = ("iq", "mag", "marker")
N, R = 16384, 4


def torch_route(ch, x, iq):
    """what a caller did with the wire frames on the device: decode_mag_16iq_le (gui.py:250-260), then max / argmax"""
    ch.process_q15(x, out=iq)
    re, im = iq[..., 0].float(), iq[..., 1].float()
    mag = torch.sqrt(re * re + im * im)
    peak, idx = mag.max(dim=1)
    return mag, peak, idx


class OtherLib:
    """sa_process_q15 of another build of the library on a handle of its own, set up like the chain beside it"""

    def __init__(self, path, sos14):
        self.L = L = C.CDLL(path if os.path.isabs(path) else os.path.join(ROOT, "fpga_real_time_fft_analyzer_amd", path))
        H = C.c_void_p
        L.sa_create.argtypes = [C.c_int, C.POINTER(H)]
        L.sa_set_filter_mode.argtypes = [H, C.c_uint8]
        L.sa_load_sos_q14.argtypes = [H, C.POINTER(C.c_int16), C.c_int]
        L.sa_process_q15.argtypes = [H, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.sa_set_profiling.argtypes = [H, C.c_int]
        L.sa_profile_read.argtypes = [H, C.POINTER(C.c_float), C.c_int]
        L.sa_reserve.argtypes = [H, C.c_int]
        L.sa_destroy.argtypes = [H]
        self.h = H()
        assert L.sa_create(0, C.byref(self.h)) == 0
        s = np.ascontiguousarray(sos14, np.int16)
        assert L.sa_load_sos_q14(self.h, s.ctypes.data_as(C.POINTER(C.c_int16)), s.shape[0]) == 0

    def timed(self, mode, xs, outs, calls, st):
        L, h = self.L, self.h
        assert L.sa_set_filter_mode(h, mode) == 0 and L.sa_set_profiling(h, calls) == 0
        for i in range(calls):
            assert L.sa_process_q15(h, xs[i % R].data_ptr(), outs[i % R].data_ptr(), xs[0].shape[0], st) == 0
        buf = (C.c_float * calls)()
        got = L.sa_profile_read(h, buf, calls)
        assert got == calls and L.sa_set_profiling(h, 0) == 0
        return [buf[i] * 1e3 for i in range(got)]

    def close(self):
        self.L.sa_destroy(self.h)


def spread(rounds):
    m = [float(np.median(r)) for r in rounds]
    return f"median {np.median(np.concatenate(rounds)):7.1f} us  round medians {min(m):.1f}-{max(m):.1f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--ab", default=None, help="another build of the library: its sa_process_q15 against this tree's iq kind")
    a = ap.parse_args()
    B = a.batch
    sos14 = np.load(os.path.join(ROOT, "tests", "golden", "g4_q15_frames.npz"))["sos_q14"]
    ch = SpectrumChain(0)
    ch.load_sos_q14(sos14)
    ch.reserve(B)
    other = OtherLib(a.ab, sos14) if a.ab else None
    if other:
        other.L.sa_reserve(other.h, B)
    gen = torch.Generator(device="cuda").manual_seed(2)
    xs = [torch.randint(-2048, 2048, (B, N), generator=gen, device="cuda", dtype=torch.int32).to(torch.int16) for _ in range(R)]
    outs = {k: [ch.process_q15(xs[r], out_kind=k) for r in range(R)] for k in KINDS}
    st = torch.cuda.current_stream().cuda_stream
    print(f"device {torch.cuda.get_device_name(0)}  B = {B}  rounds {a.rounds} x {a.calls} calls  rotating buffers {R}", flush=True)
    for mode in (0xB1, 0x00, 0xA2):
        ch.set_filter_mode(mode)
        if other:                                                # same bytes from both builds before anything is timed
            o2 = torch.empty_like(outs["iq"][0])
            assert other.L.sa_set_filter_mode(other.h, mode) == 0
            assert other.L.sa_process_q15(other.h, xs[0].data_ptr(), o2.data_ptr(), B, st) == 0
            assert torch.equal(o2, ch.process_q15(xs[0], out=outs["iq"][0])), "the two builds disagree on the wire frames"
        # the routes agree before they are compared
        pm, pb, bp = ch.markers_q15(xs[0])
        tm, tp, _ = torch_route(ch, xs[0], outs["iq"][0])        # (torch leaves open which index a tie reports)
        assert torch.equal(pm, tp) and torch.equal(tm.gather(1, pb.long()[:, None])[:, 0], pm), "marker != torch route"
        assert torch.equal(bp, (outs["iq"][0].to(torch.int64) ** 2).sum(dim=(1, 2))), "band power != torch sum"
        assert torch.equal(ch.process_q15(xs[0], out_kind="mag"), tm), "mag != torch decode"
        del tm
        t0 = time.perf_counter()                                 # sustained pre-warm: measure at the settled clock
        while time.perf_counter() - t0 < 0.5:
            for k in KINDS:
                ch.process_q15(xs[0], out=outs[k][0], out_kind=k)
            torch.cuda.synchronize()
        dev = {k: [] for k in KINDS + ("iq_other",)}
        wall = {k: [] for k in KINDS + ("iq+torch",)}
        for rnd in range(a.rounds):
            order = list(KINDS) + (["iq_other"] if other else [])
            order = order[rnd % len(order):] + order[:rnd % len(order)]          # rotate: no kind always runs first
            for k in order:
                if k == "iq_other":
                    dev[k].append(other.timed(mode, xs, outs["iq"], a.calls, st))
                    continue
                ch.set_profiling(a.calls)
                for i in range(a.calls):
                    ch.process_q15(xs[i % R], out=outs[k][i % R], out_kind=k)
                dev[k].append([t * 1e3 for t in ch.profile_read(a.calls)])
                ch.set_profiling(0)
            for k in list(KINDS) + ["iq+torch"]:
                for i in range(3):
                    torch_route(ch, xs[i % R], outs["iq"][i % R]) if k == "iq+torch" else ch.process_q15(xs[i % R], out=outs[k][i % R], out_kind=k)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(a.calls):
                    if k == "iq+torch":
                        torch_route(ch, xs[i % R], outs["iq"][i % R])
                    else:
                        ch.process_q15(xs[i % R], out=outs[k][i % R], out_kind=k)
                torch.cuda.synchronize()
                wall[k].append([(time.perf_counter() - t0) / a.calls * 1e6])
        for k in KINDS + (("iq_other",) if other else ()):
            print(f"mode 0x{mode:02X} device {k:9s} {spread(dev[k])}", flush=True)
        for k in KINDS + ("iq+torch",):
            print(f"mode 0x{mode:02X} wall   {k:9s} {spread(wall[k])}", flush=True)
        w = {k: float(np.median(np.concatenate(wall[k]))) for k in wall}
        d = {k: float(np.median(np.concatenate(dev[k]))) for k in dev if dev[k]}
        print(f"mode 0x{mode:02X} ratios: iq+torch / marker (wall) {w['iq+torch'] / w['marker']:.2f}x   "
              f"mag / iq (device) {d['mag'] / d['iq']:.3f}   marker / iq (device) {d['marker'] / d['iq']:.3f}"
              + (f"   iq / iq_other (device) {d['iq'] / d['iq_other']:.4f}" if other else ""), flush=True)
    if other:
        other.close()
    ch.close()


if __name__ == "__main__":
    main()
