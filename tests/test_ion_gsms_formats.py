"""CPU tests of the ION_GSMS layout (gsh_ion_*, include/gnss_sdr_hip.h).  The reference as compiled cannot be the yardstick everywhere (signed words,
fields across words, the MS tables: the header lists the deviations), so gsh_ion_decode_host -- the host build of the decoder the kernel shares -- is held
to the numpy restatement (tests/ion_gsms_reference.py) over a grid of layouts packed by an independent packer, to the worked examples as literals, and
to what the reference does define: its encoding tables and its block's output on inputs inside a rule fixed in advance (tests/golden/ion_gsms.npz,
minted by tests/golden/make_golden_ion_gsms.py).  Refusals, the metadata parser, the recording reader, the kernel's resources and a stand-alone
sanitizer run of the header's host decoder complete the file.  Everything is integer-exact."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import ion_gsms_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def layout_of(chunks):
    from gnss_sdr_amd.ion_gsms import IonLayout
    return IonLayout(chunks, R.flat(chunks))


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def check_against_restatement(chunks, n_cycles, seed, only=None):
    """pack known fields, decode every stream (or `only`) over windows that start and end inside a cycle with the library, compare with the restatement
    and with the values of the packed codes"""
    rng = np.random.default_rng(seed)
    fields = R.random_fields(chunks, n_cycles, rng)
    data = R.pack(chunks, n_cycles, fields, rng)
    assert data.size == n_cycles * R.cycle_bytes(chunks)
    lay = layout_of(chunks)
    try:
        assert lay.cycle_bytes == R.cycle_bytes(chunks)
        for i, s in enumerate(R.flat(chunks)):
            if only is not None and i not in only:
                continue
            exp = R.decode(chunks, data, i)
            rate = s["rate_factor"]
            assert lay.stream_info(i) == (rate, s["format"] != R.REAL, R.field_bits(s))
            assert exp.size == n_cycles * rate
            # the first field of the block holds code 0 ... and is what the packer was given
            v0 = R.value_of(s["encoding"], R.code_bits(s), R.field_to_code(s, int(fields[i][0][0])))
            first = exp[0].real if s["format"] == R.IQ else exp[0].imag if s["format"] == R.QI else exp[0]
            neg = s["negate"] & (2 if s["format"] == R.QI else 1)
            assert first == (-v0 if neg else v0), (i, s)
            for f, n in R.windows(rate, exp.size):
                got = lay.decode_host(i, data, f, n)
                assert got.dtype == exp.dtype and np.array_equal(bits(got), bits(exp[f:f + n])), (i, s, f, n)
    finally:
        lay.close()


@pytest.mark.parametrize("head", [0, 1], ids=["no_padding", "head_padding"])
@pytest.mark.parametrize("big", [0, 1], ids=["little", "big"])
@pytest.mark.parametrize("size_word", [1, 2, 4, 8])
def test_decode_host_equals_the_restatement_over_the_grid(gsh, size_word, big, head):
    """word sizes x endianness x head padding, each with widths 1..16 x real / IQ / QI x all eleven encodings (alignments 0, 1, 2 cycling), an unselected
    5-bit stream between every two, so that fields start at every bit and straddle 8-, 16-, 32- and 64-bit words"""
    for w in range(1, 17):
        for kind in (R.REAL, R.IQ, R.QI):
            c = R.grid_chunk(size_word, big, head, w, kind)
            if w >= 12 and kind != R.REAL:
                word = 8 * size_word                    # this chunk has a field across a word boundary at every word size
                pos, crossed = 0 if not head else 8 * size_word * c["count_words"] - sum(s["packed_bits"] for s in c["streams"]), False
                for s in c["streams"]:
                    fw = R.field_bits(s)
                    for j in range(R.fields_per_cycle(s)):
                        crossed |= (pos + j * fw) // word != (pos + j * fw + fw - 1) // word
                    pos += s["packed_bits"]
                assert crossed
            check_against_restatement([c], 5, 1000 * size_word + 100 * big + 10 * head + w)


def test_three_chunks_of_different_words_per_cycle(gsh):
    for w, kind in ((3, R.IQ), (7, R.REAL), (12, R.QI), (16, R.IQ)):
        chunks = [R.grid_chunk(2, 0, 1, w, kind, 0, range(0, 4)), R.grid_chunk(8, 1, 0, w, kind, 1, range(4, 8)), R.grid_chunk(1, 0, 0, w, kind, 2, range(8, 11))]
        check_against_restatement(chunks, 4, 77 + w)


@pytest.mark.parametrize("nbytes", [3, 6, 20, 4096])
def test_cycle_sizes(gsh, nbytes):
    """cycles of 3, 6, 20 and 4096 bytes: 12-bit complex TC across 8-bit words, the same twice, a 20-byte chunk of 32-bit words with 5-bit OBA, and the
    largest cycle, 512 64-bit words holding 2048 real 16-bit fields"""
    if nbytes == 3:
        chunks = [R.chunk(1, 3, [R.stream(24, 1, 12, R.TC, R.IQ)])]
    elif nbytes == 6:
        chunks = [R.chunk(1, 3, [R.stream(24, 1, 12, R.TC, R.IQ)]), R.chunk(1, 3, [R.stream(24, 1, 12, R.TCA, R.QI)], big_endian=1)]
    elif nbytes == 20:
        chunks = [R.chunk(4, 5, [R.stream(70, 7, 5, R.OBA, R.IQ), R.stream(9, 1, 3, R.SM, R.REAL, 1), R.stream(75, 15, 5, R.MS, R.REAL)], padding=1)]
    else:
        chunks = [R.chunk(8, 512, [R.stream(16384, 1024, 16, R.OG, R.REAL), R.stream(16384, 512, 9, R.SMA, R.QI, 2)])]
    assert R.cycle_bytes(chunks) == nbytes
    check_against_restatement(chunks, 3, nbytes)


def test_worked_examples(gsh):
    """the issue's table: what the layout says (not what the reference printed where its signed words decide), plus SIGN"""
    def run(data, chunks):
        lay = layout_of(chunks)
        try:
            out = lay.decode_host(0, np.array(data, np.uint8))
            assert np.array_equal(bits(out), bits(R.decode(chunks, np.array(data, np.uint8), 0)))
            return out.tolist()
        finally:
            lay.close()
    assert run([0x1B], [R.chunk(1, 1, [R.stream(8, 4, 2, R.TC)])]) == [0, 1, -2, -1]
    assert run([0x1B], [R.chunk(1, 1, [R.stream(8, 2, 2, R.SM, R.IQ)])]) == [0 + 1j, 0 - 1j]
    assert run([0x1B, 0xE4], [R.chunk(2, 1, [R.stream(16, 8, 2, R.OB)])]) == [1, 0, -1, -2, -2, -1, 0, 1]
    assert run([0xAB, 0xCD, 0xEF], [R.chunk(1, 3, [R.stream(24, 1, 12, R.TC, R.IQ)])]) == [-1348 - 529j]
    assert run([0x34, 0x12, 0xCD, 0xAB], [R.chunk(4, 1, [R.stream(24, 1, 12, R.TC, R.IQ)])]) == [-1348 - 750j]
    assert run([0x80, 0x7F], [R.chunk(1, 2, [R.stream(16, 1, 8, R.TC, R.IQ)])]) == [-128 + 127j]
    assert run([0xA5], [R.chunk(1, 1, [R.stream(8, 8, 1, R.SIGN)])]) == [-1, 1, -1, 1, 1, -1, 1, -1]


def test_header_carries_the_layout_and_keeps_the_abi():
    from gnss_sdr_amd import _lib
    assert C.sizeof(_lib.IonChunk) == 24 and C.sizeof(_lib.IonStream) == 32
    hdr = open(os.path.join(ROOT, "include", "gnss_sdr_hip.h")).read()
    for name, value in (("GSH_ABI_VERSION", 25), ("GSH_ION_MAX_CHUNKS", 16), ("GSH_ION_MAX_STREAMS", 64), ("GSH_ION_MAX_SELECTED", 8),
                        ("GSH_ION_MAX_CYCLE_BYTES", 4096)) + tuple((f"GSH_ION_{n}", i) for i, n in enumerate(R.ENCODING_NAMES + ["FP"])):
        assert f"#define {name} {value}" in hdr, name
    from gnss_sdr_amd.ion_gsms import ENCODINGS
    assert [ENCODINGS[n] for n in R.ENCODING_NAMES] == list(range(11)) and ENCODINGS["FP"] == 11


# ------------------------------------------------------------------------------------------------------------------------ golden
GOLDEN = os.path.join(HERE, "golden", "ion_gsms.npz")
IRREGULAR_MS = [3, 4, 5]     # widths at which the reference's MS table repeats its 2-bit row (ion_gsms_stream_encodings.h:125,140,155)


def test_closed_forms_equal_the_reference_tables_except_ms_at_3_4_5():
    g = np.load(GOLDEN)
    differ = []
    for q in (2, 3, 4, 5):
        table = g[f"table_{q}"]
        assert table.shape == (11, 1 << q)
        for enc in range(1, 11):
            if R.encoding_row(enc, q) != table[enc].tolist():
                differ.append((enc, q))
    assert differ == [(R.MS, q) for q in IRREGULAR_MS]
    for q in IRREGULAR_MS:      # ... and there the reference repeats its 2-bit row
        assert g[f"table_{q}"][R.MS].tolist() == [0, 0, 1, -1] * (1 << (q - 2))


def _golden_cases():
    g = np.load(GOLDEN)
    import json
    return g, json.loads(str(g["cases"]))


def test_golden_reference_block_outputs(gsh):
    """the reference block's own output on inputs inside the rule (make_golden_ion_gsms.py states it): decode_host equals it"""
    g, cases = _golden_cases()
    assert len(cases) >= 40
    seen = set()
    for k, case in enumerate(cases):
        chunks = case["chunks"]
        data = g[f"data_{k}"]
        lay = layout_of(chunks)
        try:
            for i in case["selected"]:
                s = R.flat(chunks)[i]
                exp = g[f"out_{k}_{i}"].astype(np.int64)           # the reference's items in its own order: fields as they lie in the file
                got = lay.decode_host(i, data)
                if s["format"] != R.REAL:
                    got = got.view(np.float32)
                assert np.array_equal(got.astype(np.int64), exp), (case["what"], i)
                seen.add((s["encoding"], R.field_bits(s)))
        finally:
            lay.close()
    whats = " ".join(c["what"] for c in cases)
    for enc in range(1, 11):
        for w in (2, 3, 4, 5):
            assert (enc, w) in seen or (enc == R.MS and w in IRREGULAR_MS), (enc, w)
    assert (R.TC, 8) in seen and (R.TC, 16) in seen and (R.TC, 12) in seen
    for needed in ("head padding", "skipped stream", "two chunks"):
        assert needed in whats, needed


# ------------------------------------------------------------------------------------------------------------------------ refusals
def _refused(chunks, streams=None):
    from gnss_sdr_amd import GshError
    from gnss_sdr_amd.ion_gsms import IonLayout
    with pytest.raises(GshError) as e:
        IonLayout(chunks, R.flat(chunks) if streams is None else streams)
    return e.value.code, str(e.value)


def test_descriptor_refusals(gsh):
    ok = lambda **kw: R.stream(**{**dict(packed_bits=8, rate_factor=2, quantization=4, encoding=R.TC), **kw})
    one = lambda s, **kw: [R.chunk(**{**dict(size_word=1, count_words=2, streams=[s]), **kw})]
    layout_of(one(ok())).close()                         # the base case is fine
    invalid = [
        ("size_word 3", one(ok(), size_word=3), "size_word 3"),
        ("size_word 16", one(ok(), size_word=16), "size_word 16"),
        ("count_words 0", one(ok(), count_words=0), "count_words 0"),
        ("big_endian 2", one(ok(), big_endian=2), "big_endian 2"),
        ("shift 2", one(ok(), shift=2), "shift 2"),
        ("padding 2", one(ok(), padding=2), "padding 2"),
        ("more bits than the words hold", one(ok(packed_bits=24, quantization=12), count_words=2), "hold 24 bits"),
        ("a cycle above 4096 bytes", one(ok(), size_word=8, count_words=513), "more than 4096 bytes"),
        ("packed_bits 0", one(ok(packed_bits=0)), "packed_bits 0"),
        ("rate_factor 0", one(ok(rate_factor=0)), "rate_factor 0"),
        ("an inexact division, real", one(ok(packed_bits=9, rate_factor=2, quantization=4), count_words=2), "whole number of bits"),
        ("an inexact division, complex", one(ok(packed_bits=12, rate_factor=4, quantization=1, format=R.IQ)), "whole number of bits"),
        ("a field of 17 bits", one(ok(packed_bits=17, rate_factor=1, quantization=8), count_words=3), "17 bits"),
        ("quantization 0", one(ok(quantization=0)), "quantization 0"),
        ("quantization above the field", one(ok(quantization=5)), "quantization 5"),
        ("encoding 12", one(ok(encoding=12)), "encoding 12"),
        ("encoding -1", one(ok(encoding=-1)), "encoding -1"),
        ("format 3", one(ok(format=3)), "format 3"),
        ("alignment 3", one(ok(alignment=3)), "alignment 3"),
        ("lump_shift 2", one(ok(lump_shift=2)), "lump_shift 2"),
        ("negate 4", one(ok(format=R.IQ, quantization=2, negate=4)), "negate 4"),
        ("negate Q of a real stream", one(ok(negate=2)), "negate 2"),
        ("SIGN of two bits", one(ok(encoding=R.SIGN, quantization=2, alignment=1)), "SIGN"),
        ("SIGN with the whole 4-bit field", one(ok(encoding=R.SIGN, quantization=1, alignment=0)), "SIGN"),
    ]
    for what, chunks, text in invalid:
        code, msg = _refused(chunks)
        assert code == 1 and text in msg, (what, msg)
    code, msg = _refused([R.chunk(1, 1, [ok()] * 0)] * 17, [ok()])
    assert code == 1 and "17 chunks" in msg
    code, msg = _refused([R.chunk(8, 64, [R.stream(1, 1, 1, R.SIGN)] * 65)])
    assert code == 1 and "65 streams" in msg
    c = R.chunk(1, 2, [ok()])
    c["n_streams"] = 2
    code, msg = _refused([c], [ok()])
    assert code == 1 and "n_streams 2" in msg
    unsupported = [
        ("chunk shift Right", one(ok(), shift=1), "word shift Right"),
        ("lump shift Right", one(ok(lump_shift=1)), "lump shift Right"),
        ("FP", one(ok(encoding=R.FP)), "FP"),
    ]
    for what, chunks, text in unsupported:
        code, msg = _refused(chunks)
        assert code == 5 and text in msg, (what, msg)
    # a descriptor that also breaks a rule is invalid, not unsupported
    assert _refused(one(ok(quantization=9), shift=1))[0] == 1


def test_selection_refusals_need_no_device(gsh):
    """unequal rates, mixed kinds, a stream twice or out of range and more than 8 streams are refused before any device is touched: the device
    index below does not exist"""
    from gnss_sdr_amd import GshError
    streams = [R.stream(8, 2, 2, R.TC, R.IQ), R.stream(8, 4, 2, R.TC), R.stream(16, 4, 2, R.TC, R.QI)] + [R.stream(8, 2, 2, R.OB, R.IQ)] * 9
    chunks = [R.chunk(4, 26, streams)]
    lay = layout_of(chunks)
    dst = [4096 + 64 * i for i in range(9)]
    try:
        for what, sel, text, inverted in (
                ("unequal rates", [0, 2], "2 and 4 samples per cycle", 0),
                ("mixed kinds", [0, 1], "complex and real", 0),
                ("a stream twice", [0, 3, 0], "named twice", 0),
                ("a stream out of range", [0, 12], "outside 0..11", 0),
                ("nine streams", [0, 3, 4, 5, 6, 7, 8, 9, 10], "9 streams selected", 0),
                ("no stream", [], "0 streams selected", 0),
                ("inverted_spectrum with real streams", [1], "inverted_spectrum", 1)):
            with pytest.raises(GshError) as e:
                lay.unpack_device(1 << 20, 4096, 0, 16, sel, dst[:len(sel)], bool(inverted))
            assert e.value.code == 1 and text in str(e.value), (what, str(e.value))
        with pytest.raises(GshError) as e:
            lay.unpack_device(1 << 20, 4098, 0, 16, [0], dst[:1])
        assert e.value.code == 1 and "4-byte aligned" in str(e.value)
        with pytest.raises(GshError) as e:
            lay.unpack_device(1 << 20, 4096, 0, 16, [0], [4100])
        assert e.value.code == 1 and "8-byte aligned" in str(e.value)
        assert lay.bytes_for(0, 0) == 0 and lay.bytes_for(0, 1) == 104 and lay.bytes_for(0, 2) == 104 and lay.bytes_for(2, 5) == 208
    finally:
        lay.close()


# ------------------------------------------------------------------------------------------------------------------------ metadata, recording
METADATA = """<?xml version="1.0" encoding="UTF-8"?>
<Metadata xmlns="http://www.ion.org/standards/sdrwg/schema/metadata.xsd">
  <Stream id="L1"><RateFactor>2</RateFactor><Quantization>4</Quantization><PackedBits>16</PackedBits><Alignment>Left</Alignment>
    <Format>QI</Format><Encoding>TC</Encoding></Stream>
  <stream id="L2"><ratefactor>2</ratefactor><quantization>3</quantization><packedbits>16</packedbits><alignment>Right</alignment>
    <format>InQ</format><encoding>SM</encoding></stream>
  <STREAM id="IF5"><RATEFACTOR>4</RATEFACTOR><QUANTIZATION>2</QUANTIZATION><PACKEDBITS>12</PACKEDBITS><ENCODING>OBA</ENCODING></STREAM>
  <stream id="inferred"><ratefactor>1</ratefactor><quantization>2</quantization><packedbits>4</packedbits><encoding>OB</encoding></stream>
  <Lump id="lumpA"><Stream id="L1"/><Stream id="L2"/><Shift>Left</Shift></Lump>
  <Chunk id="c0"><SizeWord>4</SizeWord><CountWords>1</CountWords><Endian>Big</Endian><Padding>None</Padding><WordShift>Left</WordShift>
    <Lump id="lumpA"/></Chunk>
  <Block id="b0"><Cycles>CYCLES</Cycles><SizeHeader>5</SizeHeader><SizeFooter>3</SizeFooter>
    <Chunk id="c0"/>
    <Chunk><SizeWord>2</SizeWord><CountWords>2</CountWords><Endian>Little</Endian><Padding>Head</Padding>
      <Lump><Stream id="IF5"/><Stream id="inferred"/><Stream id="IFn"><RateFactor>1</RateFactor><Quantization>8</Quantization><PackedBits>8</PackedBits>
        <Format>IFn</Format><Encoding>TC</Encoding></Stream></Lump></Chunk>
  </Block>
  <Lane id="lane0"><Block id="b0"/></Lane>
  <File><Url>capture.dat</Url><Offset>7</Offset><Lane id="lane0"/></File>
</Metadata>
"""


def test_metadata_parser(gsh):
    from gnss_sdr_amd.ion_gsms import IonGsmsMetadata, parse_format
    md = IonGsmsMetadata.parse(METADATA.replace("CYCLES", "4"))
    assert md.files == [{"url": "capture.dat", "offset": 7, "lane": "lane0"}]
    (block,) = md.lanes["lane0"]
    assert (block["cycles"], block["sizeheader"], block["sizefooter"]) == (4, 5, 3)
    c0, c1 = block["chunks"]
    assert (c0["size_word"], c0["count_words"], c0["big_endian"], c0["padding"], c0["shift"], c0["n_streams"]) == (4, 1, 1, 0, 0, 2)
    assert (c1["size_word"], c1["count_words"], c1["big_endian"], c1["padding"], c1["n_streams"]) == (2, 2, 0, 1, 3)
    l1, l2 = c0["streams"]
    assert (l1["name"], l1["rate_factor"], l1["quantization"], l1["packed_bits"], l1["alignment"], l1["format"], l1["negate"], l1["encoding"]) == \
        ("L1", 2, 4, 16, 1, R.QI, 0, "TC")
    assert (l2["name"], l2["alignment"], l2["format"], l2["negate"], l2["encoding"]) == ("L2", 2, R.IQ, 1, "SM")
    if5, inferred, ifn = c1["streams"]
    assert (if5["format"], if5["alignment"]) == (R.REAL, 0)            # 12 < 2 x 4 x 2: real (libs/ion_gsms_chunk_data.cc:60)
    assert inferred["format"] == R.IQ                                   # 4 >= 2 x 1 x 2: complex
    assert (ifn["format"], ifn["negate"]) == (R.REAL, 1)
    for text, expect in (("IF", (0, 0)), ("IFn", (0, 1)), ("IQ", (1, 0)), ("IQn", (1, 2)), ("InQ", (1, 1)), ("InQn", (1, 3)), ("QI", (2, 0)),
                         ("QIn", (2, 1)), ("QnI", (2, 2)), ("QnIn", (2, 3)), ("qni", (2, 2))):
        assert parse_format(text) == expect, text
    with pytest.raises(ValueError):
        parse_format("II")
    with pytest.raises(ValueError):
        IonGsmsMetadata.parse("<metadata><lane id='x'><block id='nowhere'/></lane></metadata>")


def _recording_chunks():
    return [R.chunk(4, 1, [R.stream(16, 2, 4, R.TC, R.QI, 1, name="L1"), R.stream(16, 2, 3, R.SM, R.IQ, 2, negate=1, name="L2")], big_endian=1),
            R.chunk(2, 2, [R.stream(12, 4, 2, R.OBA, name="IF5"), R.stream(4, 1, 2, R.OB, R.IQ, name="inferred"),
                           R.stream(8, 1, 8, R.TC, negate=1, name="IFn")], padding=1)]


@pytest.mark.parametrize("cycles", [4, 0])
def test_recording_reads_whole_cycles_without_headers_and_footers(gsh, tmp_path, cycles):
    from gnss_sdr_amd.ion_gsms import IonGsmsRecording
    chunks = _recording_chunks()
    cb = R.cycle_bytes(chunks)
    assert cb == 8
    rng = np.random.default_rng(5 + cycles)
    if cycles:
        blocks = [rng.integers(0, 256, cycles * cb, dtype=np.uint8) for _ in range(3)]
        body = b"".join(b"HEAD!" + b.tobytes() + b"FTR" for b in blocks) + b"HEAD!" + b"\x01" * 9      # a fourth block that is not whole
        payload = np.concatenate(blocks)
    else:
        payload = rng.integers(0, 256, 11 * cb, dtype=np.uint8)
        body = b"HEAD!" + payload.tobytes() + b"\x02" * 5 + b"FTR"                                          # 5 bytes short of a cycle, then the footer
    (tmp_path / "capture.dat").write_bytes(b"OFFSET!" + body)
    (tmp_path / "capture.sdrx").write_text(METADATA.replace("CYCLES", str(cycles)))
    rec = IonGsmsRecording(str(tmp_path / "capture.sdrx"), streams="L2, IFn")
    try:
        assert rec.layout.cycle_bytes == cb and rec.streams == [1, 4] and rec.layout.names == ["L1", "L2", "IF5", "inferred", "IFn"]
        assert rec.total_cycles == (12 if cycles else 11) and rec.samples("L2") == 2 * rec.total_cycles
        got = [rec.read(3)] + list(rec.runs(5))
        assert [g.size // cb for g in got] == ([3, 5, 4] if cycles else [3, 5, 3]) and rec.remaining == 0 and rec.read(1).size == 0
        data = np.concatenate(got)
        assert np.array_equal(data, payload[:rec.total_cycles * cb])
        for name, i in (("L2", 1), ("IFn", 4), ("L1", 0)):
            assert np.array_equal(bits(rec.layout.decode_host(name, data)), bits(R.decode(chunks, data, i))), name
    finally:
        rec.close()


# ------------------------------------------------------------------------------------------------------------------------ the kernel, the header
def test_unpack_kernel_uses_no_scratch_and_at_most_128_vgprs(gsh):
    import gnss_sdr_amd
    from kernel_metadata import kernels
    found = {n: k for n, k in kernels(gnss_sdr_amd._lib.LIB_PATH).items() if "unpack_ion_kernel" in n}
    assert len(found) == 1, list(found)
    for n, k in found.items():
        assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_count"] <= 128, (n, k[".private_segment_fixed_size"], k[".vgpr_count"])


def test_host_decoder_under_the_sanitizers(tmp_path):
    """tests/host/test_ion_decode.cc, a stand-alone program over csrc/ion_gsms.h, built with the address and undefined-behaviour sanitizers and run
    directly: a shift by the operand's width or a byte read outside the block would stop it"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    probe = tmp_path / "probe.cc"
    probe.write_text("int main() { return 0; }\n")
    # the runtimes linked statically: the program then runs whatever else the environment loads in front of it
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    r = subprocess.run([gxx] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("the sanitizer runtime is not installed: " + (r.stderr.strip().splitlines() or ["g++ failed"])[-1][:200])
    exe = tmp_path / "test_ion_decode"
    src = os.path.join(HERE, "host", "test_ion_decode.cc")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "gnss-sdr_amd", "csrc")]
    r = subprocess.run([gxx] + flags + inc + [src, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "ion decode: ok" in r.stdout, r.stdout[-1000:]
