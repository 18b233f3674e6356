"""CPU tests of the packed front-end formats (gsh_packed_format, include/gnss_sdr_hip.h): the numpy restatement of the reference's unpack
blocks (tests/packed_reference.py) equals the reference's own compiled blocks (tests/golden/packed_formats.npz, minted by
tests/golden/make_golden_packed.py) for every byte and 16-bit item value; the ctypes layout matches the header; gsh_packed_bytes sizes and
refuses without a GPU; PackedFormat.from_signal_source takes the reference's property names and defaults."""
import ctypes as C
import os

import numpy as np
import pytest

import packed_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "packed_formats.npz")
BYTES = np.arange(256, dtype=np.uint8)
ITEMS = np.arange(65536, dtype="<u2").view(np.uint8)   # every 16-bit item, little-endian in memory


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("beb", [0, 1])
@pytest.mark.parametrize("rev", [0, 1])
def test_unpack_2bit_samples_equals_reference_block(golden, beb, rev):
    assert np.array_equal(R.unpack_2bit_samples(BYTES, beb, 1, True, rev), golden[f"u2_byte_beb{beb}_rev{rev}"])
    assert np.array_equal(R.unpack_2bit_samples(ITEMS, beb, 2, True, rev), golden[f"u2_short_beb{beb}_rev{rev}"])


def test_byte_unpack_blocks_equal_reference_blocks(golden):
    assert np.array_equal(R.unpack_byte_2bit_cpx_samples(BYTES), golden["u2cpx"])
    assert np.array_equal(R.unpack_byte_4bit_samples(BYTES), golden["u4"])
    assert np.array_equal(R.unpack_byte_2bit_samples(BYTES).view(np.uint32), golden["nsr"].view(np.uint32))
    assert np.array_equal(R.unpack_ntlab_2bit_samples(BYTES).view(np.uint32), golden["ntlab"].view(np.uint32))


def test_value_sets_of_the_families():
    assert set(np.unique(R.source_output("Nsr_File_Signal_Source", BYTES))) == {-2.0, -1.0, 0.0, 1.0}
    assert set(np.unique(R.source_output("NTLab_File_Signal_Source", BYTES))) == {-3.0, -1.0, 1.0, 3.0}
    four = R.source_output("Four_Bit_Cpx_File_Signal_Source", BYTES)
    assert set(np.unique(four.real)) == set(range(-15, 16, 2))
    # Two_Bit_Cpx: two I/Q swaps -- sample 0 of byte 0b11_01_00_10 is (bits 7:6, bits 5:4) = (-1, 1) -> (2s+1) = (-1, 3)
    x = R.source_output("Two_Bit_Cpx_File_Signal_Source", np.array([0b11010010], np.uint8))
    assert x[0] == complex(-1, 3) and x[1] == complex(1, -3)


def test_packed_format_struct_matches_header():
    from gnss_sdr_amd._lib import PackedFormat
    assert C.sizeof(PackedFormat) == 32
    for i, name in enumerate(("family", "sample_type", "item_size", "big_endian_bytes", "big_endian_items", "rf_channels", "channel", "reserved")):
        assert getattr(PackedFormat, name).offset == 4 * i, name
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gnss_sdr_hip.h")).read()
    for name, value in (("GSH_PACKED_TWO_BIT", 1), ("GSH_PACKED_TWO_BIT_CPX", 2), ("GSH_PACKED_FOUR_BIT_CPX", 3), ("GSH_PACKED_NSR", 4),
                        ("GSH_PACKED_NTLAB", 5), ("GSH_PACKED_REAL", 0), ("GSH_PACKED_IQ", 1), ("GSH_PACKED_QI", 2)):
        assert f"#define {name} {value}" in hdr, name


def test_from_signal_source_defaults():
    from gnss_sdr_amd.sample_stream import PackedFormat as P
    f = P.from_signal_source("Two_Bit_Packed_File_Signal_Source")
    assert (f.family, f.sample_type, f.item_size, f.big_endian_items, f.big_endian_bytes) == (P.TWO_BIT, P.REAL, 1, 1, 0)
    f = P.from_signal_source("Two_Bit_Packed_File_Signal_Source", item_type="short", sample_type="qi", big_endian_items="false", big_endian_bytes="true",
                             filename="x.bin", sampling_frequency=20e6)
    assert (f.sample_type, f.item_size, f.big_endian_items, f.big_endian_bytes) == (P.QI, 2, 0, 1)
    assert P.from_signal_source("Four_Bit_Cpx_File_Signal_Source").sample_type == P.IQ
    assert P.from_signal_source("Two_Bit_Cpx_File_Signal_Source").is_complex
    nt = P.from_signal_source("NTLab_File_Signal_Source")
    assert (nt.family, nt.rf_channels, nt.channel) == (P.NTLAB, 4, 0)
    with pytest.raises(ValueError):
        P.from_signal_source("Labsat_Signal_Source")
    with pytest.raises(ValueError):
        P.from_signal_source("Nsr_File_Signal_Source", item_type="short")


@pytest.mark.parametrize("src", R.COMPLEX_SOURCES + R.REAL_SOURCES, ids=R.source_id)
def test_packed_bytes_sizes(gsh, src):
    from gnss_sdr_amd.sample_stream import PackedFormat, packed_bytes
    impl, props = src
    fmt = PackedFormat.from_signal_source(impl, **props)
    data = ITEMS[:1024]
    n = np.asarray(R.source_output(impl, data, **props)).shape[-1]   # samples per RF channel the reference makes of 1024 bytes
    assert fmt.samples_per_byte * 1024 == n
    assert packed_bytes(fmt, n) == 1024
    assert packed_bytes(fmt, 0) == 0


def test_packed_bytes_refusals(gsh):
    from gnss_sdr_amd import GshError
    from gnss_sdr_amd.sample_stream import PackedFormat as P, packed_bytes

    def refused(fmt, n, text):
        with pytest.raises(GshError) as e:
            packed_bytes(fmt, n)
        assert e.value.code == 1 and text in str(e.value), str(e.value)

    refused(P.from_signal_source("Two_Bit_Packed_File_Signal_Source"), 6, "whole number of input items")                 # 4 per byte
    refused(P.from_signal_source("Two_Bit_Packed_File_Signal_Source", item_type="short", sample_type="iq"), 6, "whole number")  # 4 per item
    refused(P.from_signal_source("Two_Bit_Cpx_File_Signal_Source"), 3, "whole number")
    for nch in (1, 2):
        refused(P.from_signal_source("NTLab_File_Signal_Source", RF_channels=nch), 4, "only 4")
    refused(P(99), 4, "unknown packed family")
    refused(P(P.TWO_BIT, item_size=3), 4, "item_size 3")
    refused(P(P.NSR, item_size=2), 4, "item_size 2")
    refused(P(P.NTLAB, rf_channels=4, channel=4), 4, "channel 4")
    refused(P(P.FOUR_BIT_CPX, sample_type=P.REAL), 4, "iq / qi")
    f = P.from_signal_source("Nsr_File_Signal_Source").struct()
    f.reserved = 1
    out = C.c_uint64(0)
    assert gsh.gsh_packed_bytes(C.byref(f), 4, C.byref(out)) == 1
    assert gsh.gsh_packed_bytes(None, 4, C.byref(out)) == 1
