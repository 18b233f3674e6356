"""CPU tests of the LabSat 4 families of gsh_packed_format (GSH_PACKED_LS4_1BIT .. _12BIT, include/gnss_sdr_hip.h).  No golden vector exists: as for
LabSat 3 Wideband the reference as compiled reads two bits above the layout it documents (labsat23_source.cc:67-74, a stated deviation), so the decoder
is held to the numpy restatement (tests/ls4_reference.py), to the worked examples as literals and to an independent packer that is built from codes.
gsh_packed_decode_host, the host build of the decoder every device path shares, equals the restatement; gsh_packed_bytes sizes and refuses without a
GPU; PackedFormat reads the .ini of a recording the way the reference does.  Everything is integer-exact."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import ls4_reference as L

HERE = os.path.dirname(os.path.abspath(__file__))


def P():
    from gnss_sdr_amd.sample_stream import PackedFormat
    return PackedFormat


def c64(pairs):
    return np.array([complex(i, q) for i, q in pairs], np.complex64)


def slots(regs):
    return [s for s in range(3) if regs[s]]


def _id(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


def test_header_carries_the_families_and_keeps_the_abi():
    from gnss_sdr_amd._lib import PackedFormat
    assert C.sizeof(PackedFormat) == 32
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "gnss_sdr_hip.h")).read()
    for name, value in (("GSH_PACKED_LS4_1BIT", 14), ("GSH_PACKED_LS4_2BIT", 15), ("GSH_PACKED_LS4_4BIT", 16), ("GSH_PACKED_LS4_8BIT", 17),
                        ("GSH_PACKED_LS4_12BIT", 18), ("GSH_ABI_VERSION", 25)):
        assert f"#define {name} {value}" in hdr, name
    p = P()
    assert (p.LS4_1BIT, p.LS4_2BIT, p.LS4_4BIT, p.LS4_8BIT, p.LS4_12BIT) == (14, 15, 16, 17, 18)
    assert (L.LS4_1BIT, L.LS4_2BIT, L.LS4_4BIT, L.LS4_8BIT, L.LS4_12BIT) == (14, 15, 16, 17, 18)
    f = p.ls4(12, (12, 6, 3), 2)
    s = f.struct()
    assert (s.family, s.sample_type, s.item_size, s.big_endian_bytes, s.big_endian_items, s.rf_channels, s.channel, s.reserved) == (18, 1, 8, 12, 6, 3, 2, 3)


def test_unpack_kernel_uses_no_scratch_and_at_most_128_vgprs(gsh):
    import gnss_sdr_amd
    from kernel_metadata import kernels
    found = {n: k for n, k in kernels(gnss_sdr_amd._lib.LIB_PATH).items() if "unpack_ls4_kernel" in n}
    assert len(found) == 1, list(found)
    for n, k in found.items():
        assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_count"] <= 128, (n, k[".private_segment_fixed_size"], k[".vgpr_count"])


def worked_examples():
    p = P()
    u = 1 / 2048
    return [
        ("QUA 1", 1, p.ls4(1, (1,)), np.array([0x8000000000000000], "<u8"), c64([(-1, 1)] + [(1, 1)] * 31)),
        ("QUA 2", 2, p.ls4(2, (1,)), np.array([0x6C00000000000000], "<u8"), c64([(1.0, -1.0), (-0.5, 0.5)] + [(0.5, 0.5)] * 14)),
        ("QUA 12", 12, p.ls4(12, (3,)), np.array([0x0000000000000010, 0xFF00000000000000, 0], "<u8"),
         c64([(u, u), (u, u), (2 * u, 256 * u)] + [(u, u)] * 5)),
    ]


def test_worked_examples_as_literals(gsh):
    from gnss_sdr_amd.sample_stream import packed_decode_host
    for name, qua, fmt, reg, want in worked_examples():
        ref = L.decode(reg.view(np.uint8), qua, fmt.ls4_regs, 0)
        assert np.array_equal(ref, want), (name, ref)
        got = packed_decode_host(fmt, reg.view(np.uint8), 0, want.size)
        assert np.array_equal(got, want), (name, got)


@functools.lru_cache(maxsize=None)
def packed_case(qua, regs):
    """(codes I, codes Q, the file's bytes) of ROUNDS rounds: every code appears (the first samples of every slot walk through all of them)"""
    rng = np.random.default_rng(100 * qua + sum(r << (4 * i) for i, r in enumerate(regs)))
    ci, cq = [None] * 3, [None] * 3
    for s in slots(regs):
        n = L.ROUNDS * L.samples_per_round(qua, regs, s)
        ci[s], cq[s] = rng.integers(0, 1 << qua, n), rng.integers(0, 1 << qua, n)
        walk = np.arange(min(n, 1 << qua))
        ci[s][:walk.size], cq[s][:walk.size] = walk, walk[::-1]
    return ci, cq, L.pack(ci, cq, qua, regs)


@pytest.mark.parametrize("regs", L.LAYOUTS, ids=_id)
@pytest.mark.parametrize("qua", L.QUAS)
def test_packer_round_trip(gsh, qua, regs):
    from gnss_sdr_amd.sample_stream import packed_decode_host
    ci, cq, data = packed_case(qua, regs)
    assert data.size == L.ROUNDS * L.round_bytes(regs) and (regs != (12, 6, 3) or L.round_bytes(regs) == 168)
    for s in slots(regs):
        want = (L.value(ci[s], qua) + 1j * L.value(cq[s], qua)).astype(np.complex64)
        assert want.size == L.ROUNDS * regs[s] * 32 // qua
        assert np.array_equal(L.decode(data, qua, regs, s), want), s
        assert np.array_equal(packed_decode_host(P().ls4(qua, regs, s), data, 0, want.size), want), s


@pytest.mark.parametrize("qua", L.QUAS)
def test_mapping_over_every_code(gsh, qua):
    """all 2^QUA codes (4 096 at QUA 12) as I and, reversed, as Q of one slot: generate_mapping written out with integers"""
    from gnss_sdr_amd.sample_stream import packed_decode_host
    n, half = 1 << qua, 1 << (qua - 1)
    n_samples = max(n, L.samples_per_register(qua) * (3 if qua != 12 else 1))
    regs = (n_samples * 2 * qua // 64, 0, 0)
    codes = np.arange(n_samples) % n
    data = L.pack([codes, None, None], [codes[::-1], None, None], qua, regs)
    want = np.array([(c + 1 if c < half else c - n) for c in range(n)], np.float64) / half
    assert want.min() == -1.0 and want.max() == 1.0 and np.all(want * half == np.round(want * half)) and not np.any(want == 0)
    for got in (L.decode(data, qua, regs, 0), packed_decode_host(P().ls4(qua, regs[:1]), data, 0, n_samples)):
        assert np.array_equal(got.real, want[codes].astype(np.float32)) and np.array_equal(got.imag, want[codes[::-1]].astype(np.float32))
        assert np.array_equal(got.real.astype(np.float64), want[codes])      # exact in float32


def random_registers(qua, regs, seed):
    """ROUNDS rounds of one-hot, all-ones, zero and random registers"""
    per = sum(regs)
    rnd = np.random.default_rng(seed).integers(0, 1 << 64, L.ROUNDS * per, dtype=np.uint64)
    rnd[:min(64, rnd.size)] = (np.uint64(1) << np.arange(64, dtype=np.uint64))[:min(64, rnd.size)]
    rnd[-2:] = (0xFFFFFFFFFFFFFFFF, 0)
    return rnd.astype("<u8").view(np.uint8)


def windows(qua, S, total):
    """(first, n): at 1, inside a register, at samples 2 and 5 of a triple, one before and one after a round boundary; counts that end mid-register"""
    spr = L.samples_per_register(qua)
    firsts = sorted({0, 1, 2, 5, spr - 1, spr + 1, S - 1, S + 1, 2 * S + 5})
    out = []
    for first in firsts:
        for n in sorted({1, 2, spr + 1, S, S + spr // 2 + 1, total - first}):
            if 0 < n and first + n <= total:
                out.append((first, n))
    return out


@pytest.mark.parametrize("regs", L.LAYOUTS, ids=_id)
@pytest.mark.parametrize("qua", L.QUAS)
def test_decode_host_equals_restatement(gsh, qua, regs):
    from gnss_sdr_amd.sample_stream import packed_decode_host
    data = random_registers(qua, regs, 17 * qua + sum(regs))
    for s in slots(regs):
        fmt = P().ls4(qua, regs, s)
        want = L.decode(data, qua, regs, s)
        S = L.samples_per_round(qua, regs, s)
        assert want.size == L.ROUNDS * S and fmt.ls4_samples_per_round() == S
        for first, n in windows(qua, S, want.size):
            assert np.array_equal(packed_decode_host(fmt, data, first, n), want[first:first + n]), (s, first, n)


def test_packed_bytes_sizes(gsh):
    from gnss_sdr_amd.sample_stream import packed_bytes
    p = P()
    for qua in L.QUAS:
        spr = L.samples_per_register(qua)
        for regs in L.LAYOUTS:
            for s in slots(regs):
                fmt = p.ls4(qua, regs, s)
                S = L.samples_per_round(qua, regs, s)
                assert fmt.samples_per_item == spr and fmt.item_bytes == (24 if qua == 12 else 8) and fmt.is_complex and fmt.is_register_family
                assert packed_bytes(fmt, 0) == 0
                assert packed_bytes(fmt, 123 * S) == 123 * L.round_bytes(regs)
                assert packed_bytes(fmt, spr) == L.round_bytes(regs)                 # ends inside the first round: the round's bytes
                assert packed_bytes(fmt, 4 * S + spr) == 5 * L.round_bytes(regs)
    assert [p.ls4(q, (3,)).samples_per_item for q in L.QUAS] == [32, 16, 8, 4, 8]
    with pytest.raises(ValueError):
        p.ls4(2, (6, 6, 6)).samples_per_byte


def test_packed_bytes_refusals(gsh):
    from gnss_sdr_amd import GshError
    from gnss_sdr_amd.sample_stream import packed_bytes
    p = P()

    def refused(fmt, n, *texts):
        with pytest.raises(GshError) as e:
            packed_bytes(fmt, n)
        assert e.value.code == 1 and all(t in str(e.value) for t in texts), str(e.value)

    # a partial register or triple
    refused(p.ls4(2, (6,)), 17, "17 samples are not a whole number of 8-byte registers", "16 samples")
    refused(p.ls4(8, (6, 6, 6), 1), 6, "6 samples are not a whole number of 8-byte registers", "4 samples")
    refused(p.ls4(12, (6,)), 4, "4 samples are not a whole number of 24-byte triples of registers", "8 samples")
    refused(p.ls4(12, (6,)), 12, "12 samples are not a whole number of 24-byte triples")
    # QUA 12 takes whole triples of registers in every slot
    refused(p.ls4(12, (4,)), 8, "QUA 12 with 4 registers in slot A", "multiple of 3")
    refused(p.ls4(12, (6, 5, 3), 0), 8, "QUA 12 with 5 registers in slot B")
    # rf_channels, the selected slot
    for nch in (0, 4):
        refused(p(p.LS4_2BIT, p.IQ, 8, 6, 0, rf_channels=nch), 16, f"rf_channels {nch}", "1..3 channel slots")
    refused(p.ls4(2, (0, 6, 0), 0), 16, "channel 0 (slot A) is not recorded", "register count is 0")
    refused(p.ls4(2, (6, 6, 0), 2), 16, "channel 2 (slot C) is not recorded")
    refused(p.ls4(2, (6, 6), 2), 16, "channel 2 outside 0..1")
    refused(p.ls4(2, (6, 6), -1), 16, "channel -1 outside 0..1")
    refused(p(p.LS4_2BIT, p.IQ, 8, 6, 6, rf_channels=1), 16, "register count 6 of slot B", "rf_channels 1")
    # a negative or absurd register count
    refused(p.ls4(2, (-6,)), 16, "register count -6 of slot A outside 0..1048576")
    refused(p.ls4(4, (6, 6, -1), 0), 16, "register count -1 of slot C")
    refused(p.ls4(1, ((1 << 20) + 1,)), 32, "register count 1048577 of slot A")
    # item_size, sample_type
    refused(p(p.LS4_2BIT, p.IQ, 4, 6, rf_channels=1), 16, "item_size 4", "8-byte")
    refused(p(p.LS4_12BIT, p.IQ, 24, 6, rf_channels=1), 8, "item_size 24", "8-byte")
    refused(p(p.LS4_2BIT, p.QI, 8, 6, rf_channels=1), 16, "sample_type 2", "GSH_PACKED_IQ")
    refused(p(p.LS4_8BIT, p.REAL, 8, 6, rf_channels=1), 16, "sample_type 0", "GSH_PACKED_IQ")
    # the texts of the families that were there before stand
    refused(p(99), 4, "unknown packed family 99")
    refused(p(19), 4, "unknown packed family 19")
    refused(p(p.LS3W_1BIT, p.IQ, 8, big_endian_items=True, rf_channels=1), 32, "big_endian_bytes 0 / big_endian_items 1")
    refused(p(p.LABSAT_2BIT, p.IQ, 2, flags=1), 8, "gsh_packed_format.reserved must be 0")


INI = """[config]
OSC=OCXO
SMP=61380000
QUA=12
CHN=3
BW_MAX=60000000
BW_DIV_A=1
BW_DIV_B=2
BW_DIV_C=4

[channel A]
CFA=1575420000
BWA=60000000
BUF_SIZE_A=96

[channel B]
CFB=1227600000
BWB=30000000
BUF_SIZE_B=48

[channel C]
CFC=1176450000
BWC=15000000
BUF_SIZE_C=24
"""


def test_from_ls4_ini():
    p = P()
    f = p.from_ls4_ini(INI)
    assert (f.family, f.sample_type, f.item_size, f.rf_channels, f.channel, f.ls4_regs) == (p.LS4_12BIT, p.IQ, 8, 3, 0, (12, 6, 3))
    assert (f.samples_per_item, f.item_bytes, f.ls4_round_bytes, f.ls4_samples_per_round()) == (8, 24, 168, 32)
    g = p.from_ls4_ini(INI, selected_channel=3)
    assert (g.channel, g.ls4_samples_per_round()) == (2, 8)
    cfg = p.read_ls4_ini(INI)
    assert (cfg["qua"], cfg["chn"], cfg["smp"], cfg["bw_max"], cfg["bw_div"], cfg["buf_size"]) == (12, 3, 61380000.0, 60000000, [1, 2, 4], [96, 48, 24])
    # QUAN_A where QUA is missing; one channel; a slot without a buffer
    one = "[config]\nSMP=10000000\nQUAN_A=4\nCHN=1\n[channel A]\nBUF_SIZE_A=65536\n"
    h = p.from_ls4_ini(one)
    assert (h.family, h.rf_channels, h.channel, h.ls4_regs, h.samples_per_item) == (p.LS4_4BIT, 3, 0, (8192, 0, 0), 8)
    only_b = p.from_ls4_ini(INI.replace("BUF_SIZE_A=96", "BUF_SIZE_A=0").replace("BUF_SIZE_C=24", ""), selected_channel=2)
    assert (only_b.channel, only_b.ls4_regs) == (1, (0, 6, 0))
    # from_signal_source dispatches on the extension, as generate_filename does
    k = p.from_signal_source("Labsat_Signal_Source", filename="rec/x.ls4", ini=INI, selected_channel=2)
    assert (k.family, k.channel, k.ls4_regs) == (p.LS4_12BIT, 1, (12, 6, 3))
    assert p.from_signal_source("Labsat_Signal_Source", filename="x.LS4", ini=INI.replace("QUA=12", "QUA=8")).family == p.LS4_8BIT
    w = p.from_signal_source("Labsat_Signal_Source", filename="x.ls3w", ini="[config]\nQUA=2\nCHN=3\n")
    assert w.family == p.LS3W_2BIT
    for bad, text in ((INI.replace("QUA=12", "QUA=3"), "QUA 3"), (INI.replace("QUA=12", "QUA=16"), "QUA 16"), (INI.replace("CHN=3", "CHN=4"), "CHN 4"),
                      (INI.replace("BUF_SIZE_B=48", "BUF_SIZE_B=52"), "BUF_SIZE_B 52 is not a multiple of 8"),
                      (INI.replace("BW_DIV_B=2", "BW_DIV_B=4"), "BUF_SIZE x BW_DIV differs"),
                      (INI.replace("BUF_SIZE_C=24", "BUF_SIZE_C=48"), "BUF_SIZE x BW_DIV differs"),
                      ("[other]\nQUA=2\n", "config"), ("[config]\nCHN=1\n", "QUA")):
        with pytest.raises(ValueError, match=text):
            p.from_ls4_ini(bad)
    with pytest.raises(ValueError, match="selected_channel 3"):
        p.from_ls4_ini(INI.replace("CHN=3", "CHN=2"), selected_channel=3)
    with pytest.raises(ValueError, match="selected_channel 1.*not recorded"):
        p.from_ls4_ini(INI.replace("BUF_SIZE_A=96", "BUF_SIZE_A=0"), selected_channel=1)
    with pytest.raises(ValueError, match="QUA 3"):
        p.ls4(3, (6,))
