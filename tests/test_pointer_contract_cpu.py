"""CPU: the pointer contract of the process and filter calls (include/specan.h, "pointer contract"), through the handle-free
export sa_debug_check_pointers with made-up addresses -- nothing is dereferenced, no GPU is needed.

What a call must answer is written here, from the words of the contract, and never asked of the code under test:
  - `in` is 16-byte aligned; `out` is 16-byte aligned except for SA_OUT_MAG_HALF (4) and SA_OUT_SPEC_HALF (8);
  - [in, in + in_bytes) and [out, out + out_bytes) are disjoint; touching is fine;
  - in_bytes = B * 65536 (float32), B * 32768 (int16), B * 24576 (packed); with a hop H ((B - 1) H + 16384) * 2, packed three
    quarters of that; out_bytes = B rows of the kind.
The export returns the code of sa_check_call (csrc/sa_pointers.cpp), the one check every entry point runs before anything
else; tests/test_gpu_pointer_contract.py holds the entry points to it on the device, and tests/cpp/test_sa_pointers.cpp and
tests/cpp/test_sa_call_check.cpp run the unit under the host sanitizers."""
import pytest

from native import standalone_checks

SA_OK, SA_EINVAL, SA_ESHAPE = 0, -1, -2
N = 16384
IN_FRAME = {"f32": 65536, "i16": 32768, "p12": 24576}
SAMPLE_BYTES = {"i16": (2, 1), "p12": (3, 2)}                                      # bytes per sample, as a fraction
# kind -> (bytes of one frame's output, alignment of `out`): the tables of output kinds of include/specan.h
FLOAT_KINDS = {0: (65536, 16), 1: (8193 * 4, 4), 2: (8193 * 8, 8), 3: (65536, 16), 4: (16, 16)}
Q15_KINDS = {0: (65536, 16), 1: (65536, 16), 2: (16, 16), **{0x10 | k: ((N >> k) * 8, 16) for k in range(1, 7)}}
WIRE_ONLY = {0: (65536, 16)}                                                       # sa_process_q15: no kind, the IQ frames
FILTER_OUT = {0: (32768, 16)}                                                      # sa_filter_q15*: no kind, int16 [B,16384]
# entry point (SA_ENTRY_* = the index) -> (input form, its kinds, takes a SA_Q15_HOP_KIND word)
ENTRIES = (("sa_process_f32", "f32", FLOAT_KINDS, False), ("sa_process_f32_i16", "i16", FLOAT_KINDS, False),
           ("sa_process_f32_p12", "p12", FLOAT_KINDS, False), ("sa_process_q15", "i16", WIRE_ONLY, False),
           ("sa_process_q15_out", "i16", Q15_KINDS, True), ("sa_process_q15_p12", "p12", Q15_KINDS, True),
           ("sa_filter_q15", "i16", FILTER_OUT, False), ("sa_filter_q15_p12", "p12", FILTER_OUT, False))
HOPS = (8, 4104, 16384)
OFFSETS = (1, 2, 4, 8, 12)
BASE = (1 << 47) - (1 << 36)                                                       # addresses near 2^47, 16-byte aligned


def cases():
    """Every (entry index, kind word, hop, form, frame bytes out, alignment of out) there is: each input form with each
    output kind of its chain, and for the two entry points whose word carries a hop, with each hop as well."""
    out = []
    for e, (_, form, kinds, hop_word) in enumerate(ENTRIES):
        for kind, (row, align) in kinds.items():
            for hop in (0,) + (HOPS if hop_word else ()):
                out.append((e, kind | (hop // 8) << 8, hop, form, row, align))
    return out


CASES = cases()


def in_bytes(form, hop, B):
    if hop == 0:
        return B * IN_FRAME[form]
    num, den = SAMPLE_BYTES[form]
    samples = (B - 1) * hop + N
    assert samples * num % den == 0
    return samples * num // den


def expected(form, hop, row, align, B, a_in, a_out):
    """The contract, in Python's unbounded integers."""
    n_in, n_out = in_bytes(form, hop, B), B * row
    if a_in % 16 or a_out % align:
        return SA_EINVAL
    return SA_EINVAL if a_in < a_out + n_out and a_out < a_in + n_in else SA_OK


@pytest.fixture(scope="module")
def check(hip_lib_built):
    from fpga_real_time_fft_analyzer_amd import abi
    assert tuple(name for name, *_ in ENTRIES) == abi.SA_ENTRIES
    return hip_lib_built.sa_debug_check_pointers


def test_the_matrix_is_the_one_the_contract_names():
    assert len(ENTRIES) == 8 and len(CASES) == 3 * 5 + 1 + 2 * 9 * 4 + 2
    assert sorted(k for k in Q15_KINDS if k >= 16) == [17, 18, 19, 20, 21, 22]
    assert [Q15_KINDS[0x10 | k][0] for k in (1, 4, 6)] == [65536, 8192, 2048]
    # the header's known answer: B = 5 at hop 4096 is 65536 bytes of int16 or 49152 packed, against 163840 and 122880
    assert (in_bytes("i16", 4096, 5), in_bytes("p12", 4096, 5), in_bytes("i16", 0, 5), in_bytes("p12", 0, 5)) == \
        (65536, 49152, 163840, 122880)
    assert in_bytes("i16", 16384, 5) == in_bytes("i16", 0, 5) and in_bytes("p12", 16384, 3) == in_bytes("p12", 0, 3)


def test_alignment(check):
    """`in` and `out` each off by 1, 2, 4, 8 and 12 bytes, far apart: `in` is refused at every offset, `out` exactly where the
    offset is no multiple of the kind's alignment."""
    far = BASE + (1 << 34)
    accepted = set()
    for e, word, hop, form, row, align in CASES:
        for B in (1, 3):
            assert check(e, word, BASE, far, B) == SA_OK, (e, hex(word), B)
            for off in OFFSETS:
                assert check(e, word, BASE + off, far, B) == SA_EINVAL, (e, hex(word), B, off)
                want = SA_OK if off % align == 0 else SA_EINVAL
                assert check(e, word, BASE, far + off, B) == want, (e, hex(word), B, off)
                assert check(e, word, far, BASE + off, B) == want, (e, hex(word), B, off)      # `out` below `in`
                if want == SA_OK:
                    accepted.add((e, word & 0xFF, off))
    # written out: only the two half layouts of the three float entry points take an `out` off a 16-byte boundary
    assert accepted == {(e, 1, off) for e in (0, 1, 2) for off in (4, 8, 12)} | {(e, 2, 8) for e in (0, 1, 2)}


@pytest.mark.parametrize("B", [1, 2, 5])
def test_overlap_and_touching(check, B):
    """`out` == `in`; `out` beginning one byte, one element and one frame before the end of what is read, and the mirror
    cases; touching in both orders (accepted) and one alignment step further in (refused, with both pointers aligned: by the
    overlap alone).  Every answer is the contract's, evaluated here."""
    exact = 0
    for e, word, hop, form, row, align in CASES:
        n_in, n_out = in_bytes(form, hop, B), B * row
        a_in = BASE
        tag = (e, hex(word), B)
        assert check(e, word, a_in, a_in, B) == SA_EINVAL, tag
        elem_in = 4 if form == "f32" else 2 if form == "i16" else 3
        for d in (1, align, elem_in, min(row, n_in), IN_FRAME[form]):
            for a_out in (a_in + n_in - d, a_in + d - n_out, a_in + d, a_in - d):
                want = expected(form, hop, row, align, B, a_in, a_out)
                if 0 < d <= min(n_in, n_out) and a_out in (a_in + n_in - d, a_in + d - n_out):
                    assert want == SA_EINVAL                              # d bytes are shared, whatever the alignment
                assert check(e, word, a_in, a_out, B) == want, tag + (d, a_out - a_in)
        # `out` right behind `in`: the first address behind the last byte read that `out` may have
        behind = -(-(a_in + n_in) // align) * align
        assert check(e, word, a_in, behind, B) == SA_OK, tag
        assert check(e, word, a_in, behind - align, B) == SA_EINVAL, tag          # aligned, shares the last bytes read
        if behind == a_in + n_in:
            exact += 1
            assert expected(form, hop, row, align, B, a_in, behind) == SA_OK
            assert check(e, word, a_in, behind - 1, B) == SA_EINVAL, tag          # one byte further
        else:                                                                     # a packed stream may end on 4 or 12 mod 16
            assert form == "p12" and hop and n_in % 16
        # `in` right behind `out`: out + out_bytes == in exactly (out_bytes is a multiple of the alignment)
        front = a_in - n_out
        assert front % align == 0
        assert check(e, word, a_in, front, B) == SA_OK, tag
        assert check(e, word, a_in, front + align, B) == SA_EINVAL, tag           # aligned, shares the first bytes read
        assert check(e, word, a_in, front + 1, B) == SA_EINVAL, tag               # one byte further
    assert exact >= len(CASES) - 9 * 2 and (B == 2 or exact == len(CASES))        # all but packed streams at hop 8 and 4104, B = 2


@pytest.mark.parametrize("hop", HOPS)
def test_a_hop_call_is_sized_by_its_stream(check, hop):
    """`out` inside the last N - hop samples of the stream is refused; `out` right behind the stream's last sample is
    accepted -- which for hop < N and B > 1 lies inside the bytes that B whole frames would cover: a call sized by frames
    would refuse it."""
    for e, word, h, form, row, align in CASES:
        if h != hop:
            continue
        num, den = SAMPLE_BYTES[form]
        for B in (2, 5):
            n_in = ((B - 1) * hop + N) * num // den
            assert n_in == in_bytes(form, hop, B)
            a_in, tag = BASE, (e, hex(word), B)
            end = a_in + n_in
            tail = (N - hop) * num // den                                          # bytes of the last N - hop samples
            for a_out in {(end - tail) // 16 * 16, (end - tail // 2) // 16 * 16, (end - 16) // 16 * 16}:
                if tail:
                    assert a_in <= a_out < end
                    assert check(e, word, a_in, a_out, B) == SA_EINVAL, tag + (a_out - a_in,)
            behind = -(-end // 16) * 16
            assert behind - end < 16 and check(e, word, a_in, behind, B) == SA_OK, tag
            if hop < N:
                assert behind < a_in + B * IN_FRAME[form]                          # inside what B whole frames would cover
            else:
                assert behind == a_in + B * IN_FRAME[form]
            # the frame call on the same memory reads B whole frames: the same `out` is refused there
            if hop < N:
                assert check(e, word & 0xFF, a_in, behind, B) == SA_EINVAL, tag


def test_large_batches_and_high_addresses(check):
    """B = 36 000 and 40 000 (2.4 and 2.6 GB of float frames: byte counts pass 2^31), addresses near 2^47, and intervals
    whose ends differ only above bit 31."""
    for B in (36000, 40000, 70000):
        for e, word, hop, form, row, align in CASES:
            n_in, n_out = in_bytes(form, hop, B), B * row
            tag = (e, hex(word), B)
            for a_in in (BASE, (1 << 47) - (1 << 33), 1 << 32):
                outs = [a_in + (1 << 32), a_in + (1 << 31), a_in + (1 << 31) + 16, a_in + (1 << 33), a_in + (1 << 36),
                        a_in + n_in // 16 * 16 - 16, -(-(a_in + n_in) // 16) * 16, a_in - n_out, a_in - n_out + 16,
                        a_in - (1 << 32), a_in - (1 << 31), a_in - (1 << 33), a_in - (1 << 36)]
                for a_out in outs:
                    if a_out <= 0:
                        continue
                    assert check(e, word, a_in, a_out, B) == expected(form, hop, row, align, B, a_in, a_out), \
                        tag + (hex(a_in), a_out - a_in)
    # written out for the float chain: 40 000 frames read 2 621 440 000 bytes
    assert check(0, 0, BASE, BASE + 2621440000, 40000) == SA_OK
    assert check(0, 0, BASE, BASE + 2621440000 - 16, 40000) == SA_EINVAL
    assert check(0, 0, BASE, BASE + (1 << 31), 40000) == SA_EINVAL                # 2^31 bytes in: still inside
    assert check(0, 0, BASE, BASE + (1 << 32), 40000) == SA_OK                    # equal below bit 32, 4 GiB apart
    assert check(0, 0, BASE + (1 << 32), BASE, 40000) == SA_OK
    assert check(0, 0, BASE, BASE + (1 << 32), 70000) == SA_EINVAL                # 70 000 frames read past 4 GiB
    assert check(0, 2, BASE + 40000 * 65544, BASE, 40000) == SA_OK                # spec_half writes 2 621 760 000 bytes
    assert check(0, 2, BASE + 40000 * 65544 - 16, BASE, 40000) == SA_EINVAL


def test_empty_batch_and_bad_arguments(check):
    for e, word, hop, form, row, align in CASES:
        for a_in, a_out in ((BASE, BASE), (BASE + 1, BASE + 3), (0, 0), (BASE, 0), (7, 7)):
            assert check(e, word, a_in, a_out, 0) == SA_OK, (e, hex(word))
        assert check(e, word, BASE, BASE + (1 << 34), -1) == SA_ESHAPE
        assert check(e, word, 0, BASE, 1) == SA_EINVAL and check(e, word, BASE, 0, 1) == SA_EINVAL      # NULL tensor
    far = BASE + (1 << 34)
    assert check(-1, 0, BASE, far, 1) == SA_EINVAL and check(8, 0, BASE, far, 1) == SA_EINVAL
    for e in (0, 1, 2):                                                            # the float chain: kinds 0..4, no hop
        for word in (5, -1, 17, 0x40000, 1 << 20):
            assert check(e, word, BASE, far, 1) == SA_EINVAL, (e, word)
            assert check(e, word, BASE, far, 0) == SA_EINVAL, (e, word)            # the kind is checked before the empty batch
    for e in (4, 5):
        for word in (3, 16, 23, -1, 0 | 2049 << 8, 1 << 20, 1 << 30):
            assert check(e, word, BASE, far, 1) == SA_EINVAL, (e, word)
        assert check(e, 0 | 2048 << 8, BASE, far, 1) == SA_OK
    for e in (3, 6, 7):                                                            # no kind: the word is ignored
        assert check(e, 12345, BASE, far, 1) == SA_OK


def test_standalone_program_under_host_sanitizers(tmp_path):
    """tests/cpp/test_sa_pointers.cpp + csrc/sa_pointers.cpp, host only, under the address and undefined-behaviour sanitizers
    when they link here (a plain build otherwise: the program's own checks still run)."""
    standalone_checks(tmp_path, "test_sa_pointers", ["sa_pointers.cpp"])


def test_standalone_call_check_under_host_sanitizers(tmp_path):
    """tests/cpp/test_sa_call_check.cpp + csrc/sa_pointers.cpp, built and run the same way: for each of the eleven entry
    points every rule it can reach -- code, rule and the words of sa_last_error -- the order of the rules, what the check
    decodes from an accepted call, and both exports against the check."""
    assert standalone_checks(tmp_path, "test_sa_call_check", ["sa_pointers.cpp"]) > 600

