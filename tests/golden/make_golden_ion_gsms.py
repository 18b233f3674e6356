"""Mint tests/golden/ion_gsms.npz from the reference's own ION_GSMS unpacker (src/algorithms/signal_source/libs/ion_gsms_chunk_data.cc,
ion_gsms_chunk_unpacking_ctx.h, ion_gsms_stream_encodings.h), compiled in a temporary directory against the GNU Radio and glog stand-ins of
tests/host/mock_gnuradio/ and a stand-in GnssMetadata.h that this script writes: only the accessors the unpacker uses (SizeWord, CountWords, Lumps,
Shift, Padding, Streams, Id, Packedbits, RateFactor, Quantization, Encoding).  Nothing compiled stays.  No test runs this script:
tests/test_ion_gsms_formats.py checks the library against what it wrote.  Stored:

  (a) table_2 .. table_5: the four look-up tables of encodings 1..10 (row 0 is empty there), as data;
  (b) cases / data_k / out_k_i: the output of IONGSMSChunkData::write_to_output, cycle by cycle as IONGSMSFileSource::work drives it
      (gnuradio_blocks/ion_gsms.cc:179-193), for inputs that obey a RULE FIXED IN ADVANCE -- the inputs on which the reference is well defined:
        - chunk shift Left, lump shift Left, words of 1, 2 or 4 bytes;
        - every field of a selected stream is either a whole word (8- and 16-bit TC), or has its leading bit clear and does not straddle a word:
          widths 2..5 under every encoding, TC at widths 6..16;
        - TC 12-bit in 32-bit words with any leading bit (the signed word's arithmetic shift happens to sign-extend).
      Inside the rule the cases hold: every encoding at every width 2..5 over the three word sizes, real and complex; whole-word 8- and 16-bit TC;
      head padding; a skipped stream (in every width 2..5 case: the rest of each word); two chunks per cycle.
      LEFT OUT, a deviation that include/gnss_sdr_hip.h names: MS at widths 4 and 5.  The reference's MS tables at 3, 4 and 5 bits repeat the 2-bit
      row (ion_gsms_stream_encodings.h:125,140,155); at width 3 the codes with a clear leading bit (0..3) still agree, at 4 and 5 they do not.
      A stream counts as complex where the reference infers it (packedbits >= 2 ratefactor quantization, ion_gsms_chunk_data.cc:60); its items are
      stored as the reference emits them, in file order (I, Q, I, Q ...: the cases use format IQ without negation).

The script asserts that the numpy restatement (tests/ion_gsms_reference.py) equals the reference on every stored item; a case inside the rule that
disagreed would be a new deviation to name in DESIGN.md, not to drop.

    python tests/golden/make_golden_ion_gsms.py /path/to/gnss-sdr"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ion_gsms_reference as R  # noqa: E402

METADATA_H = r"""
#ifndef STAND_IN_GNSS_METADATA_H
#define STAND_IN_GNSS_METADATA_H
#include <cstddef>
#include <string>
#include <vector>
namespace GnssMetadata
{
struct IonStream
{
    std::string id, encoding;
    std::size_t packedbits{0}, ratefactor{1}, quantization{1};
    const std::string& Id() const { return id; }
    std::size_t Packedbits() const { return packedbits; }
    std::size_t RateFactor() const { return ratefactor; }
    std::size_t Quantization() const { return quantization; }
    const std::string& Encoding() const { return encoding; }
};
struct Lump
{
    enum LumpShift { shiftLeft, shiftRight, shiftUndefined };
    std::vector<IonStream> streams;
    LumpShift shift{shiftLeft};
    const std::vector<IonStream>& Streams() const { return streams; }
    LumpShift Shift() const { return shift; }
};
struct Chunk
{
    enum WordShift { Left, Right };
    enum WordPadding { None, Head, Tail };
    std::size_t sizeword{1}, countwords{1};
    WordShift shift{Left};
    WordPadding padding{None};
    std::vector<Lump> lumps;
    std::size_t SizeWord() const { return sizeword; }
    std::size_t CountWords() const { return countwords; }
    const std::vector<Lump>& Lumps() const { return lumps; }
    WordShift Shift() const { return shift; }
    WordPadding Padding() const { return padding; }
};
}  // namespace GnssMetadata
#endif
"""

DRIVER = r"""
#include "ion_gsms_chunk_data.h"
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

// cases.txt: n_cases, then per case: n_chunks n_cycles n_selected, the selected ids, per chunk: sizeword countwords padding n_streams and per stream:
// id packedbits ratefactor quantization encoding; the bytes of case k are data_k.bin.  Output: out_k_<position among the selected>.bin, the items as
// emitted (int8 up to 8 bits, int16 above), and tables.bin.
int main(int, char** argv)
{
    const std::string dir = argv[1];
    {
        std::ofstream t(dir + "/tables.bin", std::ios::binary);
        for (int e = 0; e < 11; e++)
            for (int c = 0; c < 4; c++) t.put(static_cast<char>(GnssMetadata::two_bit_look_up<int8_t>[e][c]));
        for (int e = 0; e < 11; e++)
            for (int c = 0; c < 8; c++) t.put(static_cast<char>(GnssMetadata::three_bit_look_up<int8_t>[e][c]));
        for (int e = 0; e < 11; e++)
            for (int c = 0; c < 16; c++) t.put(static_cast<char>(GnssMetadata::four_bit_look_up<int8_t>[e][c]));
        for (int e = 0; e < 11; e++)
            for (int c = 0; c < 32; c++) t.put(static_cast<char>(GnssMetadata::five_bit_look_up<int8_t>[e][c]));
    }
    std::ifstream in(dir + "/cases.txt");
    int n_cases = 0;
    in >> n_cases;
    for (int k = 0; k < n_cases; k++)
        {
            int n_chunks = 0, n_cycles = 0, n_sel = 0;
            in >> n_chunks >> n_cycles >> n_sel;
            std::vector<std::string> ids(n_sel);
            for (auto& s : ids) in >> s;
            std::vector<GnssMetadata::Chunk> chunks(n_chunks);
            for (auto& c : chunks)
                {
                    int padding = 0, n_streams = 0;
                    in >> c.sizeword >> c.countwords >> padding >> n_streams;
                    c.padding = padding ? GnssMetadata::Chunk::Head : GnssMetadata::Chunk::None;
                    c.lumps.resize(1);
                    c.lumps[0].streams.resize(n_streams);
                    for (auto& s : c.lumps[0].streams) in >> s.id >> s.packedbits >> s.ratefactor >> s.quantization >> s.encoding;
                }
            std::vector<std::unique_ptr<IONGSMSChunkData>> data;
            std::size_t offset = 0, cycle = 0;
            std::vector<std::size_t> item_size, item_rate;
            for (const auto& c : chunks)
                {
                    data.emplace_back(new IONGSMSChunkData(c, ids, offset));
                    for (std::size_t i = 0; i < data.back()->output_stream_count(); i++)
                        {
                            item_size.push_back(data.back()->output_stream_item_size(i));
                            item_rate.push_back(data.back()->output_stream_item_rate(i));
                        }
                    offset += data.back()->output_stream_count();
                    cycle += c.sizeword * c.countwords;
                }
            std::vector<uint8_t> bytes(cycle * n_cycles);
            std::ifstream(dir + "/data_" + std::to_string(k) + ".bin", std::ios::binary).read(reinterpret_cast<char*>(bytes.data()), bytes.size());
            std::vector<std::vector<uint8_t>> out(offset);
            gr_vector_void_star ptr(offset);
            for (std::size_t i = 0; i < offset; i++)
                {
                    out[i].assign(item_size[i] * item_rate[i] * n_cycles + 64, 0);
                    ptr[i] = out[i].data();
                }
            std::vector<int> produced(offset, 0);
            std::size_t at = 0;
            while (at < bytes.size())
                for (auto& c : data)
                    {
                        at += c->read_from_buffer(bytes.data(), at);
                        c->write_to_output(ptr, produced);
                    }
            for (std::size_t i = 0; i < offset; i++)
                {
                    std::ofstream o(dir + "/out_" + std::to_string(k) + "_" + std::to_string(i) + ".bin", std::ios::binary);
                    o.put(static_cast<char>(item_size[i]));
                    o.write(reinterpret_cast<const char*>(out[i].data()), item_size[i] * produced[i]);
                }
        }
    return 0;
}
"""


def _clear_leading(chunks, selected, n_cycles, rng, any_leading=()):
    """fields for every selected stream: random, the leading bit clear unless the rule allows any (the other streams and the padding: random bits)"""
    fields = {}
    for i, s in enumerate(R.flat(chunks)):
        if i not in selected:
            continue
        w = R.field_bits(s)
        hi = 1 << (w if i in any_leading else w - 1)
        f = rng.integers(0, hi, (n_cycles, R.fields_per_cycle(s)), dtype=np.int64)
        f[0, 0], f[-1, -1] = 0, hi - 1
        fields[i] = f
    return fields


def _kind(packed_bits, rate, quantization):
    return R.IQ if packed_bits >= 2 * rate * quantization else R.REAL


def _stream(w, fields, enc, cplx, name):
    """`fields` fields of w bits: real, or complex where the reference infers it (quantization = w decides: 2 w r >= 2 r w, and w r < 2 r w)"""
    assert not cplx or fields % 2 == 0
    rate = fields // 2 if cplx else fields
    s = R.stream(w * fields, rate, w, enc, R.IQ if cplx else R.REAL, name=name)
    assert _kind(s["packed_bits"], rate, w) == s["format"]
    return s


def cases():
    out = []
    # every encoding at every width 2..5: per word as many whole fields as fit, the rest of the word a skipped stream; two words, two selected streams
    for enc in range(1, 11):
        for w in (2, 3, 4, 5):
            if enc == R.MS and w in (4, 5):
                continue                                 # the named MS deviation (module docstring)
            size_word = (1, 2, 4)[(enc + w) % 3]
            word = 8 * size_word
            n = word // w
            cplx = (enc + w) % 2 == 0 and n >= 2
            if cplx and n % 2:
                n -= 1
            streams = []
            for k in range(2):
                streams.append(_stream(w, n, enc, cplx, f"sel{k}"))
                if word - n * w:
                    streams.append(R.stream(word - n * w, 1, word - n * w, R.OB, name=f"skip{k}"))
            out.append((f"{R.ENCODING_NAMES[enc]} {w}-bit {'complex' if cplx else 'real'} in {word}-bit words, skipped stream", [R.chunk(size_word, 2, streams)], ()))
    # TC at widths 6..16, leading bit clear, one field per word with the rest skipped (16- and 32-bit words)
    for w in range(6, 17):
        size_word = 2 if w % 2 else 4
        word = 8 * size_word
        n = word // w
        streams = [_stream(w, n, R.TC, False, "sel0")]
        if word - n * w:
            streams.append(R.stream(word - n * w, 1, word - n * w, R.OB, name="skip0"))
        out.append((f"TC {w}-bit real in {word}-bit words", [R.chunk(size_word, 1, streams)], ()))
    # whole-word fields: any leading bit
    out.append(("whole-word TC 8-bit complex", [R.chunk(1, 2, [_stream(8, 2, R.TC, True, "sel0")])], (0,)))
    out.append(("whole-word TC 8-bit real", [R.chunk(1, 3, [_stream(8, 3, R.TC, False, "sel0")])], (0,)))
    out.append(("whole-word TC 16-bit complex", [R.chunk(2, 2, [_stream(16, 2, R.TC, True, "sel0")])], (0,)))
    out.append(("whole-word TC 16-bit real", [R.chunk(2, 1, [_stream(16, 1, R.TC, False, "sel0")])], (0,)))
    # TC 12-bit complex in a 32-bit word, 8 bits of tail padding, any leading bit
    out.append(("TC 12-bit complex in 32-bit words, any leading bit", [R.chunk(4, 1, [_stream(12, 2, R.TC, True, "sel0")])], (0,)))
    # head padding: 4 bits in front of three 4-bit fields; 8 bits in front of a 12-bit complex sample
    out.append(("head padding, TC 4-bit in 16-bit words", [R.chunk(2, 1, [_stream(4, 3, R.TC, False, "sel0")], padding=1)], ()))
    out.append(("head padding, OBA 3-bit complex in 32-bit words", [R.chunk(4, 1, [_stream(3, 8, R.OBA, True, "sel0")], padding=1)], ()))
    # two chunks per cycle: 8-bit words with 2-bit SM, 32-bit words with 5-bit OG and a skipped stream between two selected ones
    out.append(("two chunks per cycle, skipped stream",
                [R.chunk(1, 2, [_stream(2, 4, R.SM, True, "sel0"), _stream(2, 4, R.TCA, False, "sel1")]),
                 R.chunk(4, 2, [_stream(5, 6, R.OG, True, "sel2"), R.stream(2, 1, 2, R.OB, name="skip0"), _stream(5, 6, R.SMA, False, "sel3"),
                                R.stream(2, 1, 2, R.OB, name="skip1")])], ()))
    return out


def main(reference):
    libs = os.path.join(reference, "src", "algorithms", "signal_source", "libs")
    rng = np.random.default_rng(20241)
    n_cycles = 6
    store, meta = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "GnssMetadata.h"), "w") as f:
            f.write(METADATA_H)
        with open(os.path.join(tmp, "driver.cc"), "w") as f:
            f.write(DRIVER)
        all_cases = cases()
        lines = [str(len(all_cases))]
        for k, (what, chunks, any_leading) in enumerate(all_cases):
            flat = R.flat(chunks)
            selected = [i for i, s in enumerate(flat) if s["name"].startswith("sel")]
            data = R.pack(chunks, n_cycles, _clear_leading(chunks, selected, n_cycles, rng, any_leading), rng)
            data.tofile(os.path.join(tmp, f"data_{k}.bin"))
            lines.append(f"{len(chunks)} {n_cycles} {len(selected)} " + " ".join(flat[i]["name"] for i in selected))
            for c in chunks:
                lines.append(f"{c['size_word']} {c['count_words']} {c['padding']} {len(c['streams'])}")
                for s in c["streams"]:
                    lines.append(f"{s['name']} {s['packed_bits']} {s['rate_factor']} {s['quantization']} {R.ENCODING_NAMES[s['encoding']]}")
            store[f"data_{k}"] = data
            meta.append({"what": what, "chunks": chunks, "selected": selected})
        with open(os.path.join(tmp, "cases.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        exe = os.path.join(tmp, "mint")
        subprocess.run(["g++", "-O1", "-std=c++17", "-DUSE_GLOG_AND_GFLAGS=1", "-I" + tmp, "-I" + os.path.join(ROOT, "tests", "host", "mock_gnuradio"),
                        "-I" + libs, "-o", exe, os.path.join(tmp, "driver.cc"), os.path.join(libs, "ion_gsms_chunk_data.cc")], check=True)
        subprocess.run([exe, tmp], check=True)
        t = np.fromfile(os.path.join(tmp, "tables.bin"), np.int8)
        at = 0
        for q in (2, 3, 4, 5):
            store[f"table_{q}"] = t[at:at + 11 * (1 << q)].reshape(11, 1 << q).copy()
            at += 11 * (1 << q)
        assert at == t.size
        for k, case in enumerate(meta):
            for pos, i in enumerate(case["selected"]):
                raw = np.fromfile(os.path.join(tmp, f"out_{k}_{pos}.bin"), np.uint8)
                items = raw[1:].view(np.int8 if raw[0] == 1 else np.int16).astype(np.int16)
                s = R.flat(case["chunks"])[i]
                assert items.size == n_cycles * R.fields_per_cycle(s), (case["what"], i, items.size)
                mine = R.decode(case["chunks"], store[f"data_{k}"], i)
                mine = np.ascontiguousarray(mine).view(np.float32) if s["format"] != R.REAL else mine
                assert np.array_equal(mine.astype(np.int64), items.astype(np.int64)), f"the restatement differs from the reference inside the rule: {case['what']}, stream {i}"
                store[f"out_{k}_{i}"] = items
    store["cases"] = np.array(json.dumps(meta))
    out = os.path.join(HERE, "ion_gsms.npz")
    np.savez_compressed(out, **store)
    print(f"{out}: {len(meta)} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__.strip().splitlines()[-1].strip())
    main(sys.argv[1])
