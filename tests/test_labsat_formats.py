"""CPU tests of the register families of gsh_packed_format (include/gnss_sdr_hip.h): LabSat 2 / 3, LabSat 3 Wideband (LS3W) and SPIR 1-bit.
The numpy restatement (tests/labsat_reference.py) equals the reference's own compiled SPIR block (tests/golden/spir_1bit.npz, minted by
tests/golden/make_golden_spir.py).  No golden vector exists for LS3W: the reference as compiled reads two bits above the layout it documents
(labsat23_source.cc:67-74, a stated deviation), so the decoder is held to the restatement, to the worked examples as literals and to an independent
packer.  gsh_packed_decode_host, the host build of the decoder every device path shares, equals the restatement; gsh_packed_bytes sizes and refuses
without a GPU; PackedFormat reads a LabSat header and the .ini of an LS3W recording the way the reference does.  Everything is integer-exact."""
import ctypes as C
import os

import numpy as np
import pytest

import labsat_reference as L

HERE = os.path.dirname(os.path.abspath(__file__))
ITEMS = np.arange(65536, dtype="<u2")   # every 16-bit item


def P():
    from gnss_sdr_amd.sample_stream import PackedFormat
    return PackedFormat


def ls3w_fmt(qua, chn, dio, channel=0):
    p = P()
    return p(p.LS3W_1BIT + qua - 1, p.IQ, 8, rf_channels=chn, channel=channel, flags=1 if dio else 0)


def c64(pairs):
    return np.array([complex(i, q) for i, q in pairs], np.complex64)


def test_header_carries_the_families_and_keeps_the_abi():
    from gnss_sdr_amd._lib import PackedFormat
    assert C.sizeof(PackedFormat) == 32
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "gnss_sdr_hip.h")).read()
    for name, value in (("GSH_PACKED_LABSAT_2BIT", 8), ("GSH_PACKED_LABSAT_4BIT", 9), ("GSH_PACKED_LS3W_1BIT", 10), ("GSH_PACKED_LS3W_2BIT", 11),
                        ("GSH_PACKED_LS3W_3BIT", 12), ("GSH_PACKED_SPIR_1BIT", 13), ("GSH_ABI_VERSION", 25)):
        assert f"#define {name} {value}" in hdr, name
    p = P()
    assert (p.LABSAT_2BIT, p.LABSAT_4BIT, p.LS3W_1BIT, p.LS3W_2BIT, p.LS3W_3BIT, p.SPIR_1BIT) == (8, 9, 10, 11, 12, 13)
    assert (L.LABSAT_2BIT, L.LABSAT_4BIT, L.LS3W_1BIT, L.LS3W_2BIT, L.LS3W_3BIT, L.SPIR_1BIT) == (8, 9, 10, 11, 12, 13)


def test_spir_restatement_equals_reference_block():
    with np.load(os.path.join(HERE, "golden", "spir_1bit.npz")) as z:
        words, iq = z["words"], z["iq"]
    assert words.size == 256 + 2 + 1024 and iq.dtype == np.int16
    x = L.decode_spir_1bit(words)
    assert np.array_equal(x.real, iq[:, 0].astype(np.float32)) and np.array_equal(x.imag, iq[:, 1].astype(np.float32))
    assert set(np.unique(iq)) == {-32767, 32767}


# the worked examples: (format, register bytes, channel, expected samples)
def worked_examples():
    p = P()
    return [
        ("labsat 2-bit 0x8000", p(p.LABSAT_2BIT, p.IQ, 2), np.array([0x8000], "<u2"), c64([(1, -1)] + [(-1, -1)] * 7)),
        ("labsat 4-bit 0xB000", p(p.LABSAT_4BIT, p.IQ, 2), np.array([0xB000], "<u2"), c64([(-1, 2)] + [(1, 1)] * 3)),
        ("ls3w QUA 2 CHN 1", ls3w_fmt(2, 1, False), np.array([0x6C00000000000000], "<u8"), c64([(1.0, -1.0), (-0.5, 0.5)] + [(0.5, 0.5)] * 14)),
        ("ls3w QUA 1 CHN 1 digital I/O", ls3w_fmt(1, 1, True), np.array([0x0800000000000000], "<u8"), c64([(-1, 1)] + [(1, 1)] * 29)),
        ("ls3w QUA 3 CHN 3 channel 0", ls3w_fmt(3, 3, False), np.array([0x003FFFC000000000], "<u8"), c64([(-0.25, -0.25), (0.25, 0.25), (0.25, 0.25)])),
    ]


def test_worked_examples_as_literals(gsh):
    from gnss_sdr_amd.sample_stream import packed_decode_host
    for name, fmt, reg, want in worked_examples():
        ref = L.decode(fmt.family, reg.view(np.uint8), max(1, fmt.rf_channels), fmt.channel, bool(fmt.flags & 1))
        assert np.array_equal(ref, want), (name, ref)
        got = packed_decode_host(fmt, reg.view(np.uint8), 0, want.size)
        assert np.array_equal(got, want), (name, got)


@pytest.mark.parametrize("qua,chn,dio", L.LS3W_LAYOUTS, ids=lambda v: str(int(v)))
def test_ls3w_packer_round_trip(qua, chn, dio):
    spr, spare = L.ls3w_spr(qua, chn, dio), L.ls3w_spare(qua, chn, dio)
    assert spare in (0, 4, 8, 10) and spr * 2 * qua * chn + spare == 64
    rng = np.random.default_rng(1000 * qua + 10 * chn + int(dio))
    ci = rng.integers(0, 1 << qua, (chn, 64 * spr))
    cq = rng.integers(0, 1 << qua, (chn, 64 * spr))
    plain = L.pack_ls3w(ci, cq, qua, chn, dio)
    noisy = L.pack_ls3w(ci, cq, qua, chn, dio, rng.integers(0, 2, (64, spare)))
    assert spare == 0 or not np.array_equal(plain, noisy)
    assert np.array_equal(plain << np.uint64(spare), noisy << np.uint64(spare))   # only the spare bits differ
    for c in range(chn):
        want = (L.ls3w_value(ci[c], qua) + 1j * L.ls3w_value(cq[c], qua)).astype(np.complex64)
        assert np.array_equal(L.decode_ls3w(plain, qua, chn, dio, c), want)
        assert np.array_equal(L.decode_ls3w(noisy, qua, chn, dio, c), want), "spare bits leak into a sample"
    assert set(np.unique(L.ls3w_value(np.arange(1 << qua), qua) * 4)) <= set(range(-4, 5))   # multiples of 0.25


@pytest.mark.parametrize("family", [L.LABSAT_2BIT, L.LABSAT_4BIT])
def test_decode_host_equals_restatement_over_every_item(gsh, family):
    from gnss_sdr_amd.sample_stream import packed_decode_host
    fmt = P()(family, P().IQ, 2)
    want = L.decode(family, ITEMS.view(np.uint8))
    spi = L.samples_per_item(family)
    assert want.size == 65536 * spi
    assert np.array_equal(packed_decode_host(fmt, ITEMS.view(np.uint8), 0, want.size), want)
    assert np.array_equal(packed_decode_host(fmt, ITEMS.view(np.uint8), spi + 1, 3 * spi + 2), want[spi + 1:4 * spi + 3])
    assert set(np.unique(want.real)) == ({-1.0, 1.0} if family == L.LABSAT_2BIT else {-2.0, -1.0, 1.0, 2.0})


def test_decode_host_equals_restatement_spir(gsh):
    from gnss_sdr_amd.sample_stream import packed_decode_host
    with np.load(os.path.join(HERE, "golden", "spir_1bit.npz")) as z:
        words = z["words"].astype("<u4")
    fmt = P().from_signal_source("Spir_File_Signal_Source")
    assert np.array_equal(packed_decode_host(fmt, words.view(np.uint8), 0, words.size), L.decode_spir_1bit(words))
    assert np.array_equal(packed_decode_host(fmt, words.view(np.uint8), 5, 100), L.decode_spir_1bit(words)[5:105])


def ls3w_test_registers(seed):
    rnd = np.random.default_rng(seed).integers(0, 1 << 64, 512, dtype=np.uint64)
    return np.concatenate([np.uint64(1) << np.arange(64, dtype=np.uint64), np.array([0, 0xFFFFFFFFFFFFFFFF], np.uint64), rnd]).astype("<u8")


@pytest.mark.parametrize("qua,chn,dio", L.LS3W_LAYOUTS, ids=lambda v: str(int(v)))
def test_decode_host_equals_restatement_ls3w(gsh, qua, chn, dio):
    from gnss_sdr_amd.sample_stream import packed_decode_host
    regs = ls3w_test_registers(64 * qua + 8 * chn + int(dio))
    spr = L.ls3w_spr(qua, chn, dio)
    for c in range(chn):
        fmt = ls3w_fmt(qua, chn, dio, c)
        want = L.decode_ls3w(regs, qua, chn, dio, c)
        assert np.array_equal(packed_decode_host(fmt, regs.view(np.uint8), 0, want.size), want), c
        for first in (1, spr - 1, spr + 1):
            for n in (1, spr + 1, 7 * spr + spr // 2 + 1, want.size - first):
                assert np.array_equal(packed_decode_host(fmt, regs.view(np.uint8), first, n), want[first:first + n]), (c, first, n)


def test_packed_bytes_sizes(gsh):
    from gnss_sdr_amd.sample_stream import packed_bytes
    p = P()
    assert packed_bytes(p(p.LABSAT_2BIT, p.IQ, 2), 8 * 123) == 123 * 2
    assert packed_bytes(p(p.LABSAT_4BIT, p.IQ, 2), 4 * 123) == 123 * 2
    assert packed_bytes(p(p.SPIR_1BIT, p.IQ, 4), 123) == 123 * 4
    for qua, chn, dio in L.LS3W_LAYOUTS:
        fmt = ls3w_fmt(qua, chn, dio, chn - 1)
        spr = L.ls3w_spr(qua, chn, dio)
        assert fmt.samples_per_item == spr and fmt.item_bytes == 8
        assert packed_bytes(fmt, 123 * spr) == 123 * 8
        assert packed_bytes(fmt, 0) == 0
    assert (p(p.LABSAT_2BIT, p.IQ, 2).samples_per_item, p(p.LABSAT_4BIT, p.IQ, 2).samples_per_item, p(p.SPIR_1BIT, p.IQ, 4).samples_per_item) == (8, 4, 1)
    # the older families keep samples_per_byte, and the pair agrees with it
    two = p.from_signal_source("Two_Bit_Cpx_File_Signal_Source")
    assert (two.samples_per_byte, two.item_bytes, two.samples_per_item) == (2, 1, 2)
    with pytest.raises(ValueError):
        ls3w_fmt(2, 3, False).samples_per_byte


def test_packed_bytes_refusals(gsh):
    from gnss_sdr_amd import GshError
    from gnss_sdr_amd.sample_stream import packed_bytes
    p = P()

    def refused(fmt, n, *texts):
        with pytest.raises(GshError) as e:
            packed_bytes(fmt, n)
        assert e.value.code == 1 and all(t in str(e.value) for t in texts), str(e.value)

    # a partial item or register
    refused(p(p.LABSAT_2BIT, p.IQ, 2), 12, "12 samples are not a whole number of 2-byte items")
    refused(p(p.LABSAT_4BIT, p.IQ, 2), 6, "6 samples are not a whole number of 2-byte items")
    refused(ls3w_fmt(2, 3, False), 7, "7 samples are not a whole number of 8-byte registers", "5 samples")
    refused(ls3w_fmt(1, 1, True), 32, "32 samples are not a whole number of 8-byte registers", "30 samples")
    # rf_channels, channel
    for nch in (0, 4):
        refused(ls3w_fmt(2, nch, False), 16, f"rf_channels {nch}")
    refused(ls3w_fmt(2, 2, False, channel=2), 8, "channel 2 outside 0..1")
    refused(ls3w_fmt(3, 3, False, channel=-1), 3, "channel -1")
    refused(p(p.LABSAT_2BIT, p.IQ, 2, rf_channels=2), 8, "rf_channels 2 / channel 0", "one RF channel")
    refused(p(p.SPIR_1BIT, p.IQ, 4, channel=1), 8, "rf_channels 0 / channel 1")
    # reserved: a flags word for LS3W (bit 0 only), 0 everywhere else
    refused(p(p.LS3W_2BIT, p.IQ, 8, rf_channels=1, flags=2), 16, "reserved 2", "bit 0")
    refused(p(p.LS3W_2BIT, p.IQ, 8, rf_channels=1, flags=3), 15, "reserved 3")
    refused(p(p.LABSAT_2BIT, p.IQ, 2, flags=1), 8, "gsh_packed_format.reserved must be 0")
    refused(p(p.SPIR_1BIT, p.IQ, 4, flags=1), 8, "gsh_packed_format.reserved must be 0")
    refused(p(p.GSS6450_2BIT, p.IQ, 4, rf_channels=1, flags=1), 8, "gsh_packed_format.reserved must be 0")
    # item_size, sample_type
    refused(p(p.LABSAT_2BIT, p.IQ, 1), 8, "item_size 1", "2-byte")
    refused(p(p.LS3W_1BIT, p.IQ, 4, rf_channels=1), 32, "item_size 4", "8-byte")
    refused(p(p.SPIR_1BIT, p.IQ, 1), 8, "item_size 1", "4-byte")
    refused(p(p.LABSAT_4BIT, p.QI, 2), 8, "sample_type 2", "GSH_PACKED_IQ")
    refused(p(p.LS3W_3BIT, p.QI, 8, rf_channels=1), 10, "sample_type 2", "GSH_PACKED_IQ")
    refused(p(p.SPIR_1BIT, p.REAL, 4), 8, "sample_type 0", "GSH_PACKED_IQ")
    # big_endian_*
    refused(p(p.LABSAT_2BIT, p.IQ, 2, big_endian_bytes=True), 8, "big_endian_bytes 1 / big_endian_items 0")
    refused(p(p.LS3W_1BIT, p.IQ, 8, big_endian_items=True, rf_channels=1), 32, "big_endian_bytes 0 / big_endian_items 1")
    refused(p(p.SPIR_1BIT, p.IQ, 4, big_endian_items=True), 8, "big_endian_items 1")
    # the texts of the families that were there before stand
    refused(p(99), 4, "unknown packed family 99")
    refused(p(p.TWO_BIT, item_size=3), 4, "item_size 3: 1 (byte), or 2 (short) for GSH_PACKED_TWO_BIT only")
    refused(p(p.TWO_BIT_CPX, p.IQ, rf_channels=2), 4, "one RF channel only outside NTLab")


def labsat_header(version=b"LS3", bits=2, selector=1, length=1024, section=2, preamble=b"\0" * 8):
    h = bytearray(1024)
    h[0:8] = preamble
    h[8:11] = version
    h[11] = 1
    h[12:16] = int(length).to_bytes(4, "little")
    h[16:18] = int(section).to_bytes(2, "little")
    h[18:22] = (6).to_bytes(4, "little")
    h[22], h[23], h[24], h[25], h[26], h[27] = 1, bits, selector, 1, 0, 255
    return bytes(h)


def test_from_labsat_header():
    p = P()
    for version in (b"LS2", b"LS3"):
        for bits, family, spi in ((2, p.LABSAT_2BIT, 8), (4, p.LABSAT_4BIT, 4)):
            for length in (1024, 512):
                for selector in (1, 2, 3, 4):
                    fmt, off = p.from_labsat_header(labsat_header(version, bits, selector, length))
                    assert (fmt.family, fmt.sample_type, fmt.item_size, fmt.rf_channels, fmt.channel, fmt.flags) == (family, p.IQ, 2, 0, 0, 0)
                    assert off == length and fmt.samples_per_item == spi and fmt.is_complex
    f = p.from_signal_source("Labsat_Signal_Source", header=labsat_header(bits=4), selected_channel=1, filename="x.ls3")
    assert f.family == p.LABSAT_4BIT
    for bad, text in ((labsat_header(preamble=b"\0" * 7 + b"\1"), "preamble"), (labsat_header(version=b"LS4"), "version"),
                      (labsat_header(section=1), "section"), (labsat_header(bits=1), "bits per sample 1"), (labsat_header(bits=8), "bits per sample 8"),
                      (labsat_header(selector=0), "A + B"), (labsat_header(selector=5), "selector 5"), (b"\0" * 20, "20 bytes")):
        with pytest.raises(ValueError, match=text.replace("+", r"\+")):
            p.from_labsat_header(bad)
    with pytest.raises(ValueError, match="only one channel"):
        p.from_labsat_header(labsat_header(selector=1), selected_channel=2)
    with pytest.raises(ValueError, match="only one channel"):
        p.from_signal_source("Labsat_Signal_Source", header=labsat_header(selector=3), selected_channel=2)
    with pytest.raises(ValueError, match="from_labsat_header"):
        p.from_signal_source("Labsat_Signal_Source")


def test_from_ls3w_ini():
    p = P()
    ini = "[config]\nOSC=OCXO\nSMP=58000000\nQUA=2\nCHN=3\nSFT=12\n\n[channel A]\nCF=1575420000\n"
    f = p.from_ls3w_ini(ini)
    assert (f.family, f.sample_type, f.item_size, f.rf_channels, f.channel, f.flags) == (p.LS3W_2BIT, p.IQ, 8, 3, 0, 0)
    assert f.samples_per_item == 5
    f = p.from_ls3w_ini(ini.replace("QUA=2", "QUAN_A=1").replace("CHN=3", "CHN=2"), selected_channel=2, digital_io_enabled=True)
    assert (f.family, f.rf_channels, f.channel, f.flags, f.samples_per_item) == (p.LS3W_1BIT, 2, 1, 1, 15)
    # a wrong SFT is replaced by 2 QUA CHN: the layout is the same
    g = p.from_ls3w_ini(ini.replace("SFT=12", "SFT=7"), selected_channel=3)
    assert (g.family, g.rf_channels, g.channel, g.samples_per_item) == (p.LS3W_2BIT, 3, 2, 5)
    h = p.from_signal_source("Labsat_Signal_Source", ini=ini.replace("QUA=2", "QUA=3"), selected_channel=3, digital_io_enabled="true")
    assert (h.family, h.rf_channels, h.channel, h.flags, h.samples_per_item) == (p.LS3W_3BIT, 3, 2, 1, 3)
    for bad, text in ((ini.replace("QUA=2", "QUA=4"), "QUA 4"), (ini.replace("CHN=3", "CHN=4"), "CHN 4"), ("[other]\nQUA=2\n", "config"),
                      ("[config]\nCHN=1\n", "QUA")):
        with pytest.raises(ValueError, match=text):
            p.from_ls3w_ini(bad)
    with pytest.raises(ValueError, match="selected_channel 3"):
        p.from_ls3w_ini(ini.replace("CHN=3", "CHN=2"), selected_channel=3)


def test_from_signal_source_spir():
    p = P()
    f = p.from_signal_source("Spir_File_Signal_Source")
    assert (f.family, f.sample_type, f.item_size, f.rf_channels, f.channel, f.flags) == (p.SPIR_1BIT, p.IQ, 4, 0, 0, 0)
    g = p.from_signal_source("Spir_File_Signal_Source", item_type="gr_complex", filename="x.dat")   # falls back to int, as the reference does
    assert (g.family, g.item_size) == (p.SPIR_1BIT, 4)
    assert f.is_complex and f.samples_per_item == 1 and f.item_bytes == 4
