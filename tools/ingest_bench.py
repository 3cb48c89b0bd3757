#!/usr/bin/env python3
"""N3 measured: host int16 sample stream -> FrameCutter -> pinned double buffer (DeviceFeeder) -> Q15 path.

Reports frames/s end to end and the host->device rate against the PCIe bound DESIGN.md quotes (63 GB/s spec:
1.97 M int16 frames/s), for (a) numpy batches copied into the pinned staging buffers by the feeder (what a
socket / file reader delivers) and (b) the same with the host copy taken out (samples produced in pinned
memory).  With --events it also prints, per batch, the copy and kernel intervals measured with HIP events on
their own streams, which shows the copy of batch k+1 running under the kernels of batch k.
--float: the same int16 batches into the FLOAT chain (sa_process_f32_i16, mode 0xA1 with the headline cascade): no
conversion pass on the device, the PCIe volume of the Q15 path.
--packed (implies --float): the same samples packed to 12 bits (sa_process_f32_p12, 24576 bytes per frame instead of
32768), packed once up front as the int16 batches are generated up front; the GB/s figures count the packed bytes.
--packed-q15: the packed feeder into the INTEGER chain (sa_process_q15_p12; without --float / --packed, which keep their
meaning and win when given as well): the bit-exact frames from 24576 input bytes per frame.
--hop H (the integer chain; with --packed-q15 on packed samples): overlapping frames at hop H, a multiple of 8.  The sample
stream through StreamCutter(H, batch_frames) + the stream feeder into process_q15(x, hop=H) -- every sample crosses the link
once -- against the same stream cut on the host by FrameCutter(H) + the frame feeder into the frame call, 16384 / H times
the bytes; both cut up front, 'marker' records out, the two alternating in one process over --rounds R (default 5) runs of
n_batches batches each.  Choose n_batches so that a run lasts some tenths of a second.  The bound on the ratio is 16384 / H.
--hop H --trace W --group A: the stream form alone, with the copy of the result back to pinned host memory behind every call
on the call's stream: the plain trace at bucket W (traces_q15(x, bucket=W, hop=H): 131072 / W bytes per frame back) against
the grouped one (group=A: a factor A fewer), alternating as above.
--hop H --spectra A: the same with the full-resolution spectra over groups of A frames (spectra_q15(x, A, hop=H): 131072 / A
bytes per frame back) against the grouped trace at bucket W = --trace (default 16) and the same A, a factor 16384 / W fewer.
usage: ingest_bench.py [batch_frames] [n_batches] [mode] [--events] [--float] [--packed] [--packed-q15]
                       [--hop H [--rounds R] [--trace W --group A | --spectra A [--trace W]]]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fpga_real_time_fft_analyzer_amd.chain import SpectrumChain  # noqa: E402
from fpga_real_time_fft_analyzer_amd.ingest import DeviceFeeder, FrameCutter, StreamCutter, pack12  # noqa: E402

# the box gives this job 16 CPUs of a 256-core host: torch's default intra-op pool (one thread per visible core)
# stalls the staging copy for 50-100 ms every dozen batches
torch.set_num_threads(min(8, len(os.sched_getaffinity(0))))
N = 16384
B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
NB = int(sys.argv[2]) if len(sys.argv) > 2 else 32
mode = int(sys.argv[3], 0) if len(sys.argv) > 3 and not sys.argv[3].startswith("--") else 0xB1
PACKED = "--packed" in sys.argv
FLOAT = "--float" in sys.argv or PACKED
PACKED = PACKED or ("--packed-q15" in sys.argv and not FLOAT)              # from here on: the input form alone
ROW, FRAME_BYTES = (3 * N // 2, 3 * N // 2) if PACKED else (N, 2 * N)      # elements and bytes of an input frame
IN_DT = torch.uint8 if PACKED else torch.int16



def opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def hop_mode(hop, rounds):
    """--hop: the stream form against host-cut frames, alternating"""
    ch = SpectrumChain(0)
    ch.set_filter_mode(mode)
    ch.reserve(B)
    s = np.random.default_rng(0).integers(-2048, 2048, size=(4 * B - 1) * hop + N, dtype=np.int16)
    s = pack12(s) if PACKED else s
    blocks = StreamCutter(hop, B, PACKED).push(s)                      # 4 distinct blocks of B frames, reused
    frames = FrameCutter(hop, PACKED).push(s)
    assert len(blocks) == 4 and frames.shape == (4 * B, ROW)
    batches = [frames[i * B:(i + 1) * B] for i in range(4)]
    elem = s.itemsize
    forms = {"frames": (DeviceFeeder(0, max_batch=B, packed=PACKED), batches, None, B * ROW * elem),
             "stream": (DeviceFeeder(0, max_batch=B, packed=PACKED, stream=True), blocks, hop, blocks[0].size * elem)}
    out = [torch.empty((B, 4), dtype=torch.int32, device="cuda") for _ in range(2)]

    def run(form, nb):
        feeder, data, h, _ = forms[form]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, xd in enumerate(feeder.feed(data[j & 3] for j in range(nb))):
            ch.process_q15(xd, out=out[i & 1], out_kind="marker", hop=h)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    rec = {}
    for form in forms:                                                  # warm-up, and the two forms agree
        run(form, 4)
        rec[form] = out[1].clone()
    assert torch.equal(rec["frames"], rec["stream"]), "the stream form and the host-cut frames disagree"
    rate = {form: [] for form in forms}
    for _ in range(rounds):
        for form in forms:
            rate[form].append(NB * B / run(form, NB))
    h2d = pure_h2d()
    print(f"hop {hop} ({'packed 12-bit' if PACKED else 'int16'} samples), batch {B} frames x {NB} batches per run, {rounds} "
          f"alternating runs, filter mode 0x{mode:02X}, marker records out; a frames run lasts {NB * B / np.median(rate['frames']):.2f} s")
    print(f"  pinned host -> device copy alone: {h2d / 1e9:6.1f} GB/s")
    for form, (_, _, _, nbytes) in forms.items():
        r = np.array(rate[form])
        print(f"  {form:6s}: {nbytes / B:8.0f} bytes per frame on the link; M frames/s per run "
              f"{' '.join(f'{v / 1e6:.3f}' for v in r)}; median {np.median(r) / 1e6:.3f} (max/min {r.max() / r.min():.3f}) = "
              f"{np.median(r) * nbytes / B / 1e9:5.1f} GB/s")
    ratio = np.array(rate["stream"]) / np.array(rate["frames"])
    print(f"  stream / frames per round: {' '.join(f'{v:.3f}' for v in ratio)}; median {np.median(ratio):.3f}; "
          f"the bound is 16384 / hop = {N / hop:.2f} (bytes: {forms['frames'][3] / forms['stream'][3]:.3f})")
    ch.close()


def hop_trace_mode(hop, rounds, W, A):
    """--hop H --trace W --group A: plain against grouped trace from the stream, results copied back"""
    ch = SpectrumChain(0)
    ch.set_filter_mode(mode)
    ch.reserve(B)
    s = np.random.default_rng(0).integers(-2048, 2048, size=(4 * B - 1) * hop + N, dtype=np.int16)
    s = pack12(s) if PACKED else s
    blocks = StreamCutter(hop, B, PACKED).push(s)                      # 4 distinct blocks of B frames, reused
    feeder = DeviceFeeder(0, max_batch=B, packed=PACKED, stream=True)
    forms = {"plain": None, "grouped": A}
    out = {f: [torch.empty((B // (g or 1), N // W, 2), dtype=torch.float32, device="cuda") for _ in range(2)] for f, g in forms.items()}
    host = {f: [torch.empty(o.shape, dtype=torch.float32).pin_memory() for o in out[f]] for f in forms}

    def run(form, nb):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, xd in enumerate(feeder.feed(blocks[j & 3] for j in range(nb))):
            ch.traces_q15(xd, bucket=W, out=out[form][i & 1], hop=hop, group=forms[form])
            host[form][i & 1].copy_(out[form][i & 1], non_blocking=True)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for form in forms:                                                  # warm-up (grows the grouped kind's workspace)
        run(form, 4)
    # the last block fed was blocks[3] into buffer 1 in both forms: the grouped records are the plain ones, reduced
    assert torch.equal(host["grouped"][1][..., 0], host["plain"][1][..., 0].reshape(B // A, A, N // W).amax(1))
    rate = {form: [] for form in forms}
    for _ in range(rounds):
        for form in forms:
            rate[form].append(NB * B / run(form, NB))
    print(f"hop {hop} ({'packed 12-bit' if PACKED else 'int16'} samples), batch {B} frames x {NB} batches per run, {rounds} "
          f"alternating runs, filter mode 0x{mode:02X}, trace W = {W} from the stream, result copied to pinned host memory; "
          f"a plain run lasts {NB * B / np.median(rate['plain']):.2f} s")
    for form, g in forms.items():
        r = np.array(rate[form])
        back = (N // W) * 8 / (g or 1)
        print(f"  {form:7s}{'' if g is None else f' A = {g}'}: {back:6.0f} bytes per frame back; M frames/s per run "
              f"{' '.join(f'{v / 1e6:.3f}' for v in r)}; median {np.median(r) / 1e6:.3f} (max/min {r.max() / r.min():.3f}) = "
              f"{np.median(r) * back / 1e9:5.1f} GB/s back, {np.median(r) * blocks[0].size * s.itemsize / B / 1e9:5.1f} GB/s in")
    ratio = np.array(rate["grouped"]) / np.array(rate["plain"])
    print(f"  grouped / plain per round: {' '.join(f'{v:.3f}' for v in ratio)}; median {np.median(ratio):.3f}")
    ch.close()


def hop_spectra_mode(hop, rounds, A, W):
    """--hop H --spectra A: grouped trace at bucket W against full-resolution spectra from the stream, results copied back"""
    ch = SpectrumChain(0)
    ch.set_filter_mode(mode)
    ch.reserve(B)
    s = np.random.default_rng(0).integers(-2048, 2048, size=(4 * B - 1) * hop + N, dtype=np.int16)
    s = pack12(s) if PACKED else s
    blocks = StreamCutter(hop, B, PACKED).push(s)                      # 4 distinct blocks of B frames, reused
    feeder = DeviceFeeder(0, max_batch=B, packed=PACKED, stream=True)
    forms = {"trace": N // W, "spectra": N}                             # records per row
    out = {f: [torch.empty((B // A, p, 2), dtype=torch.float32, device="cuda") for _ in range(2)] for f, p in forms.items()}
    host = {f: [torch.empty(o.shape, dtype=torch.float32).pin_memory() for o in out[f]] for f in forms}

    def run(form, nb):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, xd in enumerate(feeder.feed(blocks[j & 3] for j in range(nb))):
            if form == "trace":
                ch.traces_q15(xd, bucket=W, out=out[form][i & 1], hop=hop, group=A)
            else:
                ch.spectra_q15(xd, A, out=out[form][i & 1], hop=hop)
            host[form][i & 1].copy_(out[form][i & 1], non_blocking=True)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for form in forms:                                                  # warm-up (grows both workspaces)
        run(form, 4)
    # the last block fed was blocks[3] into buffer 1 in both forms: the trace's peaks are the spectra's, topped per bucket
    assert torch.equal(host["trace"][1][..., 0], host["spectra"][1][..., 0].reshape(B // A, N // W, W).amax(2))
    rate = {form: [] for form in forms}
    for _ in range(rounds):
        for form in forms:
            rate[form].append(NB * B / run(form, NB))
    print(f"hop {hop} ({'packed 12-bit' if PACKED else 'int16'} samples), batch {B} frames x {NB} batches per run, {rounds} "
          f"alternating runs, filter mode 0x{mode:02X}, groups of A = {A} frames from the stream, result copied to pinned host "
          f"memory; a trace run lasts {NB * B / np.median(rate['trace']):.2f} s")
    for form, p in forms.items():
        r = np.array(rate[form])
        back = p * 8 / A
        print(f"  {form:7s} {'W = ' + str(W) if form == 'trace' else 'all bins'}: {back:6.0f} bytes per frame back; M frames/s per run "
              f"{' '.join(f'{v / 1e6:.3f}' for v in r)}; median {np.median(r) / 1e6:.3f} (max/min {r.max() / r.min():.3f}) = "
              f"{np.median(r) * back / 1e9:5.1f} GB/s back, {np.median(r) * blocks[0].size * s.itemsize / B / 1e9:5.1f} GB/s in")
    ratio = np.array(rate["spectra"]) / np.array(rate["trace"])
    print(f"  spectra / trace per round: {' '.join(f'{v:.3f}' for v in ratio)}; median {np.median(ratio):.3f}")
    ch.close()


def pure_h2d():
    pin = torch.empty((B, ROW), dtype=IN_DT).pin_memory()
    dev = torch.empty((B, ROW), dtype=IN_DT, device="cuda")
    for _ in range(3):
        dev.copy_(pin, non_blocking=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        dev.copy_(pin, non_blocking=True)
    torch.cuda.synchronize()
    return 20 * B * FRAME_BYTES / (time.perf_counter() - t0)


if "--hop" in sys.argv:
    if FLOAT:
        sys.exit("--hop is a mode of the integer chain (with --packed-q15 for packed samples)")
    if "--spectra" in sys.argv:
        hop_spectra_mode(opt("--hop", N), opt("--rounds", 5), opt("--spectra", 16), opt("--trace", 16))
        sys.exit(0)
    if "--trace" in sys.argv:
        hop_trace_mode(opt("--hop", N), opt("--rounds", 5), opt("--trace", 16), opt("--group", 16))
        sys.exit(0)
    hop_mode(opt("--hop", N), opt("--rounds", 5))
    sys.exit(0)

ch = SpectrumChain(0)
if FLOAT:
    ch.load_sos(np.load(os.path.join(ROOT, "tests", "golden", "g2_config1.npz"))["sos"])
ch.set_filter_mode(mode)
ch.reserve(B)
rng = np.random.default_rng(0)
host = [rng.integers(-2048, 2048, size=(B, N), dtype=np.int16) for _ in range(4)]       # 4 distinct batches, reused
if PACKED:
    host = [pack12(b) for b in host]
out = [torch.empty((B, N) if FLOAT else (B, N, 2), dtype=torch.float32 if FLOAT else torch.int16, device="cuda")
       for _ in range(2)]
feeder = DeviceFeeder(0, max_batch=B, packed=PACKED)


def process(xd, o):
    if FLOAT:
        ch.process_f32(xd, out=o)          # int16 tensor in: sa_process_f32_i16; uint8: sa_process_f32_p12
    else:
        ch.process_q15(xd, out=o)          # int16 tensor in: sa_process_q15; uint8: sa_process_q15_p12


def run(batches):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i, xd in enumerate(feeder.feed(batches)):
        process(xd, out[i & 1])
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def pure_kernels():
    xd = torch.from_numpy(host[0]).cuda()
    for _ in range(3):
        process(xd, out[0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        process(xd, out[0])
    torch.cuda.synchronize()
    return 20 * B / (time.perf_counter() - t0)


run(host[i & 3] for i in range(4))                        # warm-up
dt = run(host[i & 3] for i in range(NB))
h2d = pure_h2d()
kfps = pure_kernels()
print(f"batch {B} frames x {NB} batches, filter mode 0x{mode:02X}")
print(f"  pinned host -> device copy alone      : {h2d / 1e9:6.1f} GB/s = {h2d / FRAME_BYTES / 1e6:5.2f} M frames/s   (PCIe Gen5 x16 spec 63 GB/s = {63e9 / FRAME_BYTES / 1e6:4.2f} M frames/s)")
print(f"  {('float chain from packed 12-bit' if PACKED else 'float chain from int16') if FLOAT else 'Q15 kernels from packed 12-bit' if PACKED else 'Q15 kernels'} alone, inputs resident: {kfps / 1e6:5.2f} M frames/s")
print(f"  feeder end to end (numpy -> pinned -> device -> path): {NB * B / dt / 1e6:5.2f} M frames/s = {NB * B * FRAME_BYTES / dt / 1e9:5.1f} GB/s of samples ({FRAME_BYTES} bytes per frame)")
# the host copy into the staging buffer is part of the feeder; how much of the time is it?
t0 = time.perf_counter()
for i in range(8):
    feeder._pinned[i & 1][:B].copy_(torch.from_numpy(host[i & 3]))
tcopy = (time.perf_counter() - t0) / 8
print(f"  host copy numpy -> pinned staging     : {tcopy * 1e3:.2f} ms per batch (torch copy_, multi-threaded)")

if "--events" in sys.argv:
    # per-batch intervals on the copy stream and on the compute stream
    cs = feeder._copy_stream
    ev = []
    torch.cuda.synchronize()
    base = torch.cuda.Event(enable_timing=True)
    base.record()
    for i in range(6):
        slot = i & 1
        feeder._pinned[slot][:B].copy_(torch.from_numpy(host[i & 3]))
        c0, c1, k0, k1 = (torch.cuda.Event(enable_timing=True) for _ in range(4))
        with torch.cuda.stream(cs):
            c0.record(cs)
            feeder._dev[slot][:B].copy_(feeder._pinned[slot][:B], non_blocking=True)
            c1.record(cs)
        torch.cuda.current_stream().wait_event(c1)
        k0.record()
        process(feeder._dev[slot][:B], out[slot])
        k1.record()
        ev.append((c0, c1, k0, k1))
    torch.cuda.synchronize()
    print("  batch   copy [ms from start]        kernels [ms from start]")
    for i, (c0, c1, k0, k1) in enumerate(ev):
        print(f"   {i}     {base.elapsed_time(c0):7.3f} .. {base.elapsed_time(c1):7.3f}      {base.elapsed_time(k0):7.3f} .. {base.elapsed_time(k1):7.3f}")
ch.close()
