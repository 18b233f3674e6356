"""CPU tests of LabSatRecording (gnss_sdr_amd/labsat.py), the host file handling of the reference's Labsat_Signal_Source: temporary recordings of the
three generations are written by the packers of tests/ls4_reference.py and tests/labsat_reference.py (LabSat 2 / 3: a header and random 16-bit items)
and read back block by block; the blocks, decoded by gsh_packed_decode_host from the first-sample index that read_block returns, equal the samples
that went in, sample for sample.  Also: the _0000.LS3 sequence and its end, seconds_to_skip into the middle of a LabSat 4 buffer, the end of the data."""
import numpy as np
import pytest

import labsat_reference as L3
import ls4_reference as L

READS = (1, 7, 64, 5, 1000, 33)      # uneven reads, cycled until the data ends


def ls4_ini(qua, regs, smp=61380000):
    divs = [max(regs) // r if r else 1 for r in regs]
    text = f"[config]\nOSC=OCXO\nSMP={smp}\nQUA={qua}\nCHN=3\nBW_MAX=60000000\n" + "".join(f"BW_DIV_{x}={d}\n" for x, d in zip("ABC", divs))
    for x, r in zip("ABC", regs):
        if r:
            text += f"\n[channel {x}]\nCF{x}=1575420000\nBW{x}=10000000\nBUF_SIZE_{x}={8 * r}\n"
    return text, divs


def write_ls4(tmp_path, qua, regs, seed=3):
    rng = np.random.default_rng(seed)
    ci, cq, want = [None] * 3, [None] * 3, [None] * 3
    for s in range(3):
        if regs[s]:
            n = L.ROUNDS * L.samples_per_round(qua, regs, s)
            ci[s], cq[s] = rng.integers(0, 1 << qua, n), rng.integers(0, 1 << qua, n)
            want[s] = (L.value(ci[s], qua) + 1j * L.value(cq[s], qua)).astype(np.complex64)
    path = tmp_path / f"rec{qua}.ls4"
    path.write_bytes(L.pack(ci, cq, qua, regs).tobytes())
    text, divs = ls4_ini(qua, regs)
    (tmp_path / f"rec{qua}.ini").write_text(text)
    return str(path), want, divs


def read_all(rec, channel=None):
    """every remaining sample through uneven read_block calls, decoded from the returned first-sample index"""
    from gnss_sdr_amd.sample_stream import packed_decode_host
    fmt = rec.format if channel is None else rec.format.with_channel(channel)
    out, k = [], 0
    while rec.remaining:
        n = min(READS[k % len(READS)], rec.remaining)
        before = rec.position
        data, first = rec.read_block(READS[k % len(READS)])
        assert rec.position == before + n and data.size % rec.round_bytes == 0
        assert first == before % rec.samples_per_round and data.size == ((first + n - 1) // rec.samples_per_round + 1) * rec.round_bytes
        out.append(packed_decode_host(fmt, data, first, n))
        k += 1
    data, first = rec.read_block(8)
    assert data.size == 0 and first == 0 and rec.remaining == 0          # the end of the data
    return np.concatenate(out)


@pytest.mark.parametrize("regs", [(12, 6, 3), (6, 6, 6), (0, 6, 0)], ids=str)
@pytest.mark.parametrize("qua", [2, 12])
def test_ls4_reads_back(gsh, tmp_path, qua, regs):
    from gnss_sdr_amd.labsat import LabSatRecording
    path, want, divs = write_ls4(tmp_path, qua, regs)
    for s in range(3):
        if not regs[s]:
            with pytest.raises(ValueError, match="not recorded"):
                LabSatRecording(path, (s + 1,))
            continue
        rec = LabSatRecording(path, (s + 1,))
        assert rec.generation == "ls4" and rec.channels == [s] and rec.format.ls4_regs == regs and rec.format.channel == s
        assert rec.sample_rate == 61380000 / divs[s] and rec.total_samples == want[s].size and rec.position == 0
        assert np.array_equal(read_all(rec), want[s]), s
    if regs == (6, 6, 6):
        rec = LabSatRecording(path, (3, 1))
        assert rec.channels == [2, 0] and rec.format.channel == 2
    if regs == (12, 6, 3):
        with pytest.raises(ValueError, match="12 and 3 registers"):
            LabSatRecording(path, (1, 3))
    with pytest.raises(ValueError, match="distinct"):
        LabSatRecording(path, (2, 2))


def test_ls4_seconds_to_skip_lands_inside_a_buffer(gsh, tmp_path):
    from gnss_sdr_amd.labsat import LabSatRecording
    smp = 61380000.0
    # QUA 12, slot A: 12 registers = 96 bytes = 32 samples a round.  77 samples are 231 bytes: 2 buffers and 39 bytes, one whole triple (24 bytes, 8
    # samples) and 15 bytes that the rounding drops: sample 72, where the reference would stand at register 4 of the buffer, inside a triple
    path, want, _ = write_ls4(tmp_path, 12, (12, 6, 3))
    rec = LabSatRecording(path, (1,), seconds_to_skip=77.5 / smp)
    assert rec.position == 72 and rec.remaining == want[0].size - 72
    assert np.array_equal(read_all(rec), want[0][72:])
    # slot C at BW_DIV 4: 3 registers = 24 bytes = 8 samples a round; 4 x 29.5 / SMP seconds are 29 samples of it, 87 bytes: 3 buffers and 15 bytes,
    # no whole triple: sample 24
    rec = LabSatRecording(path, (3,), seconds_to_skip=4 * 29.5 / smp)
    assert rec.position == 24 and np.array_equal(read_all(rec), want[2][24:])
    # QUA 2, slot B of three equal ones: 6 registers = 48 bytes = 96 samples a round.  250 samples are 125 bytes: 2 buffers and 29 bytes, 3 whole
    # registers of 16 samples: sample 240
    path, want, _ = write_ls4(tmp_path, 2, (6, 6, 6))
    rec = LabSatRecording(path, (2,), seconds_to_skip=250.5 / smp)
    assert rec.position == 240 and np.array_equal(read_all(rec), want[1][240:])
    with pytest.raises(ValueError, match="shorter"):
        LabSatRecording(path, (2,), seconds_to_skip=1.0)


def test_ls3w_reads_back(gsh, tmp_path):
    from gnss_sdr_amd.labsat import LabSatRecording
    qua, chn = 2, 3
    spr = L3.ls3w_spr(qua, chn, False)
    rng = np.random.default_rng(9)
    ci, cq = rng.integers(0, 1 << qua, (chn, 40 * spr)), rng.integers(0, 1 << qua, (chn, 40 * spr))
    (tmp_path / "wide.LS3W").write_bytes(L3.pack_ls3w(ci, cq, qua, chn, False).astype("<u8").tobytes())
    (tmp_path / "wide.ini").write_text(f"[config]\nSMP=58000000\nQUA={qua}\nCHN={chn}\nSFT=12\n")
    for c in range(chn):
        rec = LabSatRecording(str(tmp_path / "wide.LS3W"), (c + 1,))
        assert rec.generation == "ls3w" and rec.sample_rate == 58e6 and rec.total_samples == 40 * spr
        want = (L3.ls3w_value(ci[c], qua) + 1j * L3.ls3w_value(cq[c], qua)).astype(np.complex64)
        assert np.array_equal(read_all(rec), want), c
    rec = LabSatRecording(str(tmp_path / "wide.LS3W"), (2, 1))
    assert rec.channels == [1, 0]
    with pytest.raises(ValueError, match="LabSat 4 recordings only"):
        LabSatRecording(str(tmp_path / "wide.LS3W"), (1,), seconds_to_skip=0.001)
    with pytest.raises(ValueError, match="selected_channel 4"):
        LabSatRecording(str(tmp_path / "wide.LS3W"), (4,))


def labsat_header(version=b"LS3", bits=2, length=1024):
    h = bytearray(length)
    h[8:11] = version
    h[11] = 1
    h[12:16] = int(length).to_bytes(4, "little")
    h[16:18] = (2).to_bytes(2, "little")
    h[18:22] = (6).to_bytes(4, "little")
    h[22], h[23], h[24], h[25], h[26], h[27] = 1, bits, 1, 1, 0, 255
    return bytes(h)


@pytest.mark.parametrize("bits", [2, 4])
def test_ls3_sequence_of_three_files_and_ls2(gsh, tmp_path, bits):
    from gnss_sdr_amd.labsat import LabSatRecording
    family = L3.LABSAT_2BIT if bits == 2 else L3.LABSAT_4BIT
    rng = np.random.default_rng(bits)
    parts = [rng.integers(0, 65536, n).astype("<u2") for n in (37, 1, 50)]
    base = tmp_path / "drive"
    for k, items in enumerate(parts):
        (tmp_path / f"drive_{k:04d}.LS3").write_bytes((labsat_header(bits=bits, length=512) if k == 0 else b"") + items.tobytes())
    (tmp_path / "drive_0004.LS3").write_bytes(parts[0].tobytes())           # _0003 is missing: the data ends with _0002
    rec = LabSatRecording(str(base))
    assert rec.generation == "ls3" and len(rec.files) == 3 and rec.format.family == family and rec.sample_rate is None
    want = L3.decode(family, np.concatenate(parts).view(np.uint8))
    assert rec.total_samples == want.size == 88 * (8 if bits == 2 else 4)
    assert np.array_equal(read_all(rec), want)
    # a LabSat 2 file: one file, never a sequence
    (tmp_path / "old.ls2").write_bytes(labsat_header(b"LS2", bits) + parts[2].tobytes() + b"\x01")   # (a trailing half item is not read)
    (tmp_path / "old.ls2_0001.LS3").write_bytes(parts[0].tobytes())
    rec = LabSatRecording(str(tmp_path / "old.ls2"))
    assert rec.generation == "ls2" and len(rec.files) == 1
    assert np.array_equal(read_all(rec), L3.decode(family, parts[2].view(np.uint8)))
    with pytest.raises(ValueError, match="one"):
        LabSatRecording(str(base), (1, 2))
    with pytest.raises(FileNotFoundError):
        LabSatRecording(str(tmp_path / "nothing"))
