"""CPU: overlapping frames cut on the device from one sample stream (SA_Q15_HOP_KIND of include/specan.h) as far as they can
be checked without a GPU: the kind word in the header and in abi.py, numpy models of the two read sites with a frame stride
-- the 8-sample unit of the cascades' staging waves (cascade_q15.hip, q15_load_tile<HOP>) and stage 0 of the FFT
(fft_q15.hip, fx_load16 with a stride), each on int16 and on packed samples, as tests/test_q15_p12_cpu.py models them for
one frame -- and ingest.StreamCutter, which cuts the streams on the host."""
import re

import numpy as np
import pytest

from conftest import N, ROOT

P12 = 24576
HOPS = (8, 4104, 16376)         # packed frames 12 bytes apart; an odd field (packed frames alternate mod 8); the largest below N
B = 3


def header():
    return open(f"{ROOT}/include/specan.h").read()


def header_macro():
    """SA_Q15_HOP_KIND of the header as a Python function: its replacement text, with C's integer division."""
    m = re.search(r"#define SA_Q15_HOP_KIND\(kind, hop\) (.+)", header())
    assert m, "SA_Q15_HOP_KIND(kind, hop) not defined in include/specan.h"
    body = m.group(1).strip()
    assert re.fullmatch(r"[()\w\s|/<]+", body), body
    return lambda kind, hop: eval(body.replace("/", "//"), {"kind": kind, "hop": hop})


def sext12(v):
    v = np.asarray(v, np.int64) & 0xFFF
    return (v - ((v & 0x800) << 1)).astype(np.int16)


# ------------------------------------------------------------------------------------------ the kind word
def test_known_answers_in_header_and_abi_py():
    from fpga_real_time_fft_analyzer_amd import abi
    c_macro = header_macro()
    names = {"SA_Q15_OUT_IQ": 0, "SA_Q15_OUT_MAG": 1, "SA_Q15_OUT_MARKER": 2, "SA_Q15_TRACE_KIND(4)": 20}
    known = re.findall(r"SA_Q15_HOP_KIND\((SA_Q15_\w+(?:\(\d\))?), (\d+)\) = (0x[0-9a-fA-F]+)", header())
    assert len(known) >= 3, known
    for name, hop, word in known:
        kind, hop, word = names[name], int(hop), int(word, 16)
        assert c_macro(kind, hop) == word == abi.SA_Q15_HOP_KIND(kind, hop), (name, hop)
        assert word & 0xFF == kind and (word >> 8) & 0xFFF == hop // 8 and word >> 20 == 0
    # spelled out once more, independent of the header's text
    assert abi.SA_Q15_HOP_KIND(abi.SA_Q15_OUT_IQ, 8192) == 0x40000
    assert abi.SA_Q15_HOP_KIND(abi.SA_Q15_OUT_MARKER, 4096) == 0x20002
    assert abi.SA_Q15_HOP_KIND(abi.SA_Q15_TRACE_KIND(4), 8) == 0x114
    assert abi.SA_Q15_HOP_KIND(abi.SA_Q15_OUT_MAG, N) == 0x80001 and abi.SA_Q15_HOP_FIELD_MAX == N // 8 == 2048
    # the documented stream length: B = 5 at hop 4096
    m = re.search(r"#define SA_Q15_HOP_STREAM_SAMPLES\(batch, hop\) (.+)", header())
    assert m and "SA_Q15_HOP_STREAM_SAMPLES(5, 4096) = 32768" in header()
    assert (5 - 1) * 4096 + N == 32768


def test_field_zero_leaves_every_existing_code_unchanged():
    from fpga_real_time_fft_analyzer_amd import abi
    c_macro = header_macro()
    kinds = [abi.SA_Q15_OUT_IQ, abi.SA_Q15_OUT_MAG, abi.SA_Q15_OUT_MARKER] + [abi.SA_Q15_TRACE_KIND(k) for k in range(1, 7)]
    assert kinds == [0, 1, 2, 17, 18, 19, 20, 21, 22]
    for kind in kinds:
        assert c_macro(kind, 0) == kind == abi.SA_Q15_HOP_KIND(kind, 0)
        for hop in (8, 4104, N):                               # and a hop never reaches into the kind's byte
            assert c_macro(kind, hop) & 0xFF == kind and c_macro(kind, hop) == abi.SA_Q15_HOP_KIND(kind, hop)


def test_no_new_symbol_and_no_new_abi_version():
    from fpga_real_time_fft_analyzer_amd import abi
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"#define SA_ABI_VERSION 4\b", txt)
    declared = set(re.findall(r"\b(sa_\w+)\s*\(", txt))
    # 44 symbols when the hop word was added; the one export since is the pointer contract's handle-free check
    assert declared == set(abi.SIGNATURES) and len(declared) == 45
    assert len(declared - {"sa_debug_check_pointers"}) == 44


def test_null_handle_is_rejected_without_a_gpu(hip_lib_built):
    from fpga_real_time_fft_analyzer_amd import abi
    word = abi.SA_Q15_HOP_KIND(abi.SA_Q15_OUT_IQ, 8192)
    assert hip_lib_built.sa_process_q15_out(None, None, None, 1, word, None) == abi.SA_EINVAL
    assert hip_lib_built.sa_process_q15_p12(None, None, None, 1, word, None) == abi.SA_EINVAL


# ------------------------------------------------------------------------------------------ the address maps
def stream_of(hop, seed):
    """(int16 samples, the same samples packed) of a stream of B frames at `hop`"""
    from fpga_real_time_fft_analyzer_amd.ingest import pack12
    s = np.random.default_rng(seed).integers(-2048, 2048, (B - 1) * hop + N).astype(np.int16)
    return s, pack12(s)


@pytest.mark.parametrize("hop", HOPS)
def test_tile_unit_address_map_with_a_frame_stride(hop):
    """q15_load_tile<HOP>: unit u = 0..2047 of frame b is samples b hop + 8 u .. + 7.  int16: the 16 bytes at byte
    2 (b hop + 8 u), 16-byte aligned.  Packed: the 12 bytes at byte b (3 hop / 2) + 12 u, three dwords on a dword boundary
    (and, at hop = 8, on every residue mod 16), taken apart by p12_unpack8.  The last unit of the last frame ends with the
    stream."""
    s, p = stream_of(hop, hop)
    b = np.arange(B)[:, None]
    u = np.arange(N // 8)[None, :]
    want = s[(b * hop + 8 * u)[..., None] + np.arange(8)]                      # [B, 2048, 8]
    # int16
    byte = 2 * (b * hop + 8 * u)
    assert not (byte % 16).any() and byte.min() == 0 and byte[B - 1].max() + 16 == s.nbytes
    got = s.view(np.uint8)[byte[..., None] + np.arange(16)].view("<i2")
    assert np.array_equal(got, want)
    # packed
    fbase = b * (3 * hop // 2)
    byte = fbase + 12 * u
    assert (3 * hop) % 2 == 0 and not (byte % 4).any() and byte.min() == 0 and byte[B - 1].max() + 12 == p.size
    if hop == 8:
        assert sorted(set((fbase % 16).ravel().tolist())) == [0, 8, 12]                   # frames at bytes 0, 12, 24
        assert set((byte % 16).ravel().tolist()) == {0, 4, 8, 12}
    d = p.view("<u4").astype(np.uint64)
    w0, w1, w2 = d[byte // 4], d[byte // 4 + 1], d[byte // 4 + 2]
    align = lambda h, l, sh: (((h << np.uint64(32)) | l) >> np.uint64(sh)) & np.uint64(0xFFFFFFFF)
    s8 = [w0, w0 >> np.uint64(12), align(w1, w0, 24), w1 >> np.uint64(4), w1 >> np.uint64(16), align(w2, w1, 28),
          w2 >> np.uint64(8), w2 >> np.uint64(20)]
    assert np.array_equal(np.stack([sext12(x) for x in s8], axis=-1), want)


@pytest.mark.parametrize("hop", HOPS)
def test_fft_stage0_address_map_with_a_frame_stride(hop):
    """fx_load16 with a stride: thread t, m = 0..15 of frame b takes sample b hop + t + 1024 m.  int16: the 2 bytes at sample
    index b hop + t + 1024 m.  Packed: dword b (3 hop / 8) + (12 t >> 5) + 384 m at bit 12 t & 31, the next dword only where
    the sample straddles; the highest dword read in the last frame is the stream's last."""
    s, p = stream_of(hop, hop + 1)
    b = np.arange(B)[:, None, None]
    t = np.arange(1024)[None, :, None]
    m = np.arange(16)[None, None, :]
    want = s[b * hop + t + 1024 * m]                                            # [B, 1024, 16]
    # int16: sample indices, every one inside the stream, the last frame's last the stream's last
    idx = b * hop + t + 1024 * m
    assert idx.min() == 0 and idx[B - 1].max() == s.size - 1
    # packed
    assert (3 * hop) % 8 == 0
    bit = 12 * t
    sh = (bit & 31) + 0 * m
    i0 = b * (3 * hop // 8) + (bit >> 5) + 384 * m
    i1 = i0 + (sh > 20)
    ndw = p.size // 4
    assert p.size % 4 == 0 and i0.min() == 0 and i0[B - 1].max() == ndw - 1 and i1.max() == ndw - 1
    d = p.view("<u4").astype(np.uint64)
    v = (((d[i1] << np.uint64(32)) | d[i0]) >> sh.astype(np.uint64)) & np.uint64(0xFFFFFFFF)
    assert np.array_equal(sext12(v), want)


# ------------------------------------------------------------------------------------------ StreamCutter
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("hop,frames", [(4096, 5), (8192, 3), (4104, 4), (N, 2), (16376, 1)])
def test_stream_cutter_blocks_hold_the_frame_cutters_frames(hop, frames, packed):
    """Random chunkings (packed chunks may end inside a pair of samples): every block is (frames - 1) hop + N samples,
    block i begins at sample i frames hop of the stream, consecutive blocks share exactly N - hop samples, flush() yields the
    remaining complete frames, and the frames FrameCutter(hop) cuts from the blocks are those it cuts from the whole
    stream, in order, once each."""
    from fpga_real_time_fft_analyzer_amd.ingest import FrameCutter, StreamCutter, pack12
    rng = np.random.default_rng(hop + frames + packed)
    total = 3 * frames + 1                                                      # frames in the stream: three blocks and one frame
    n = (total - 1) * hop + N + 1000                                            # ... and a rest short of a hop
    s = rng.integers(-2048, 2048, n & ~1).astype(np.int16)
    st, per = (pack12(s), 3) if packed else (s, 2)                              # elements per two samples
    ref = FrameCutter(hop, packed=packed).push(st)
    assert ref.shape[0] == total
    c = StreamCutter(hop, frames, packed)
    blocks, i = [], 0
    while i < st.size:
        k = int(rng.integers(1, 30001))                                         # odd and even lengths alike
        blocks += c.push(st[i:i + k])
        i += k
    assert len(blocks) == total // frames and c.block_size == ((frames - 1) * hop + N) * per // 2
    for j, blk in enumerate(blocks):
        assert blk.ndim == 1 and blk.dtype == st.dtype and blk.size == c.block_size
        at = j * frames * hop * per // 2
        assert np.array_equal(blk, st[at:at + blk.size]), j
    ov = (N - hop) * per // 2
    for a, b in zip(blocks, blocks[1:]):
        assert np.array_equal(a[a.size - ov:], b[:ov]) and a.size - frames * hop * per // 2 == ov
    last = c.flush()
    if total % frames:                                                          # the one frame that remains
        assert last is not None and last.size == N * per // 2
        blocks.append(last)
    else:
        assert last is None
    assert c.flush() is None and c.pending < N * per // 2
    got = np.concatenate([FrameCutter(hop, packed=packed).push(blk) for blk in blocks])
    assert np.array_equal(got, ref)


def test_stream_cutter_refusals_and_short_streams():
    from fpga_real_time_fft_analyzer_amd.ingest import StreamCutter
    for hop in (0, 4, 12, N + 8, 8.0, True):
        with pytest.raises(ValueError):
            StreamCutter(hop, 4)
    for frames in (0, -1, 2.0):
        with pytest.raises(ValueError):
            StreamCutter(4096, frames)
    c = StreamCutter(4096, 4)
    assert c.push(np.zeros(N - 1, np.int16)) == [] and c.flush() is None and c.pending == N - 1
    with pytest.raises(ValueError):
        StreamCutter(4096, 4, packed=True).push(np.zeros(3, np.int16))


def test_stream_feeder_checks_its_arguments_before_it_touches_the_gpu():
    from fpga_real_time_fft_analyzer_amd.ingest import DeviceFeeder
    with pytest.raises(ValueError):
        DeviceFeeder(0, max_batch=8, stream=True, consumer_depth=5)
