"""Galileo telemetry pages on the device (csrc/telemetry_viterbi.hip through gnss_sdr_amd.telemetry) against the numpy restatement (tests/tlm_reference.py,
itself held to the reference by tests/test_tlm_reference.py): bits, CRC register and verdict, bit for bit, in both metric modes, on every page of
tests/golden/viterbi.npz; the metric carry-over of reference mode across pages, launches and a channel reset; the CRC chain; the preamble scan at every
position; and the frame synchroniser on the device.  The shapes are the real page sizes."""
import numpy as np
import pytest

import tlm_reference as R
import tlm_sync_cases as cases
from gnss_sdr_amd.telemetry import GalileoFrameSync, TelemetryDecoder

pytestmark = pytest.mark.gpu
METRICS = ["full", "reference"]


def _symbols_and_offsets():
    """every fixture page in one buffer: -> (symbols, {name: [offset per page]})"""
    parts, offsets, at = [], {}, 0
    for name, _ in R.FIXTURE_FRAMES:
        sym = R.fixture()[name + "__sym"]
        offsets[name] = [at + i * sym.shape[1] for i in range(len(sym))]
        parts.append(sym.reshape(-1))
        at += sym.size
    return np.concatenate(parts), offsets


def _register(bits, crc_bits):
    return R.crc24q(bits[:crc_bits])


def _sent(bits, crc_bits):
    return int("".join(map(str, bits[crc_bits:crc_bits + 24])), 2)


def _check(result, bits, crc_bits, where):
    assert np.array_equal(result["bits"], bits), where
    assert np.array_equal(result["words"], R.pack_bits(bits)), where
    assert result["crc_register"] == _register(bits, crc_bits), where
    assert result["crc_ok"] == int(_sent(bits, crc_bits) == _register(bits, crc_bits)), where


@pytest.mark.parametrize("metric", METRICS)
def test_one_channel_one_page_every_fixture_page(gpu, metric):
    symbols, offsets = _symbols_and_offsets()
    want = R.fixture_decoded(metric, False)   # a page on its own: in reference mode a fresh object
    dec = TelemetryDecoder(1, metric, gpu)
    for name, ft in R.FIXTURE_FRAMES:
        crc_bits = R.GEOMETRY[ft]["info_bits"] - 24
        for i, off in enumerate(offsets[name]):
            dec.channel_reset(0)
            res = dec.decode_pages(symbols, [dict(channel=0, frame_type=ft, symbol_offset=off, crc_bits=crc_bits, crc_check=1)])
            _check(res[0], want[name][i], crc_bits, (name, i))
    dec.close()


@pytest.mark.parametrize("metric", METRICS)
def test_three_channels_of_three_frame_types_interleaved_in_one_table(gpu, metric):
    """channel 2 I/NAV, channel 0 F/NAV, channel 1 C/NAV, their pages interleaved in the table: each channel's pages in table order, so reference mode
    carries each channel's metrics through its own sequence (the fixture's reused object) whatever lies between"""
    symbols, offsets = _symbols_and_offsets()
    want = R.fixture_decoded(metric, metric == "reference")
    channel = {"inav": 2, "fnav": 0, "cnav": 1}
    jobs, key = [], []
    n = len(offsets["inav"])
    for i in range(n):
        for name, ft in (R.FIXTURE_FRAMES if i % 2 else R.FIXTURE_FRAMES[::-1]):
            jobs.append(dict(channel=channel[name], frame_type=ft, symbol_offset=offsets[name][i], crc_bits=R.GEOMETRY[ft]["info_bits"] - 24, crc_check=1))
            key.append((name, i, ft))
    dec = TelemetryDecoder(3, metric, gpu)
    res = dec.decode_pages(symbols, jobs)
    for r, (name, i, ft) in zip(res, key):
        _check(r, want[name][i], R.GEOMETRY[ft]["info_bits"] - 24, (name, i))
        if metric == "reference":
            assert np.array_equal(r["bits"], R.fixture()[name + "__reused"][i]), (name, i)
    dec.close()


def _seventy_channel_table(offsets):
    """70 channels (more than a wave has lanes), 1 - 3 pages each (uneven tails), the frame type and the fixture pages varying with the channel, some jobs
    continuing the CRC register of the channel's previous job; the channels' jobs are dealt out round by round, so they interleave"""
    rng = np.random.default_rng(70)
    per_channel = []
    for c in range(70):
        name, ft = R.FIXTURE_FRAMES[c % 3]
        picks = rng.integers(0, len(offsets[name]), 1 + c % 3)
        per_channel.append([dict(channel=c, frame_type=ft, symbol_offset=offsets[name][int(p)], flags=int(rng.integers(0, 2)) | (2 if k and c % 2 else 0),
                                 crc_bits=int(rng.integers(0, R.GEOMETRY[ft]["info_bits"] - 23)), crc_check=int(rng.integers(0, 2))) for k, p in enumerate(picks)])
    return [jobs[k] for k in range(3) for jobs in per_channel[::-1] if k < len(jobs)]


@pytest.mark.parametrize("metric", METRICS)
def test_seventy_channels_host_and_device_inputs(gpu, metric):
    import torch
    symbols, offsets = _symbols_and_offsets()
    jobs = _seventy_channel_table(offsets)
    assert len({j["channel"] for j in jobs}) == 70 and len(jobs) == sum(1 + c % 3 for c in range(70))
    want = R.NumpyTelemetryDecoder(70, metric).decode_pages(symbols, jobs)
    dec = TelemetryDecoder(70, metric, gpu)
    got = dec.decode_pages(symbols, jobs)
    dec.close()
    dec = TelemetryDecoder(70, metric, gpu)
    resident = torch.from_numpy(symbols).to(f"cuda:{gpu}")
    torch.cuda.synchronize()
    got_device = dec.decode_pages_device(resident.data_ptr(), len(symbols), jobs)
    dec.close()
    for k, (w, g, d) in enumerate(zip(want, got, got_device)):
        for r in (g, d):
            assert np.array_equal(r["bits"], w["bits"]) and np.array_equal(r["words"], w["words"]), k
            assert (r["crc_register"], r["crc_ok"]) == (w["crc_register"], w["crc_ok"]), (k, jobs[k])


@pytest.mark.parametrize("name,ft", R.FIXTURE_FRAMES)
def test_reference_mode_carries_the_metrics_across_launches_and_a_reset_clears_them(gpu, name, ft):
    symbols, offsets = _symbols_and_offsets()
    jobs = [dict(channel=1, frame_type=ft, symbol_offset=off) for off in offsets[name]]
    reused, fresh = R.fixture()[name + "__reused"], R.fixture()[name + "__fresh"]
    dec = TelemetryDecoder(2, "reference", gpu)
    one = dec.decode_pages(symbols, jobs)
    dec.channel_reset(1)
    cut = len(jobs) // 2 + 1
    two = dec.decode_pages(symbols, jobs[:cut]) + dec.decode_pages(symbols, jobs[cut:])
    for i in range(len(jobs)):
        assert np.array_equal(one[i]["bits"], reused[i]) and np.array_equal(two[i]["bits"], reused[i]), (name, i)
    # the sequence differs from fresh objects somewhere (else this test shows nothing), and after a reset the next page is a fresh object's
    differ = [i for i in range(len(jobs)) if not np.array_equal(reused[i], fresh[i])]
    assert differ
    for i in differ[:3]:
        dec.channel_reset(1)
        assert np.array_equal(dec.decode_pages(symbols, [jobs[i]])[0]["bits"], fresh[i]), (name, i)
    dec.close()


def test_crc_chain_of_an_inav_word_and_single_bit_errors(gpu):
    rng = np.random.default_rng(81)
    even, odd = R.inav_word(rng)
    even_bad, odd_bad = even.copy(), odd.copy()
    even_bad[40] ^= 1
    odd_bad[60] ^= 1
    symbols = np.concatenate([R.encode_page(p, 1) for p in (even, odd, even_bad, odd_bad)])
    dec = TelemetryDecoder(2, "full", gpu)
    for flavour in ("explicit", "auto"):
        for k, (e, o, want) in enumerate([(0, 1, 1), (2, 1, 0), (0, 3, 0)]):
            if flavour == "explicit":
                jobs = [dict(channel=1, frame_type=1, symbol_offset=240 * e, crc_bits=114), dict(channel=1, frame_type=1, symbol_offset=240 * o, flags=2, crc_bits=82, crc_check=1)]
            else:
                jobs = [dict(channel=1, frame_type=1, symbol_offset=240 * e, flags=4), dict(channel=1, frame_type=1, symbol_offset=240 * o, flags=4)]
            res = dec.decode_pages(symbols, jobs)
            assert [r["crc_ok"] for r in res] == [-1, want], (flavour, k)
            # the chain also holds across launches: the odd part alone continues from the even part of the launch before
            res = dec.decode_pages(symbols, jobs[:1]) + dec.decode_pages(symbols, jobs[1:])
            assert [r["crc_ok"] for r in res] == [-1, want], (flavour, k)
    # a reset clears the chain: the odd part then runs from a zero register and fails
    dec.decode_pages(symbols, [dict(channel=1, frame_type=1, symbol_offset=0, crc_bits=114)])
    dec.channel_reset(1)
    assert dec.decode_pages(symbols, [dict(channel=1, frame_type=1, symbol_offset=240, flags=2, crc_bits=82, crc_check=1)])[0]["crc_ok"] == 0
    dec.close()


@pytest.mark.parametrize("ft", [2, 3])
def test_crc_of_fnav_and_cnav_pages_and_single_bit_errors(gpu, ft):
    rng = np.random.default_rng(82 + ft)
    good = R.nav_page(rng, ft)
    flipped_data, flipped_crc = good.copy(), good.copy()
    flipped_data[17] ^= 1
    flipped_crc[-3] ^= 1
    g = R.GEOMETRY[ft]
    symbols = np.concatenate([R.encode_page(p, ft) for p in (good, flipped_data, flipped_crc)])
    dec = TelemetryDecoder(1, "full", gpu)
    res = dec.decode_pages(-symbols, [dict(channel=0, frame_type=ft, symbol_offset=k * g["symbols"], flags=1, crc_bits=g["info_bits"] - 24, crc_check=1) for k in range(3)])
    assert [r["crc_ok"] for r in res] == [1, 0, 0]
    for r, p in zip(res, (good, flipped_data, flipped_crc)):
        assert np.array_equal(r["bits"], p)
    dec.close()


@pytest.mark.parametrize("ft", [1, 2, 3])
def test_preamble_scan_equals_numpy_at_every_position(gpu, ft):
    rng = np.random.default_rng(90 + ft)
    pre = R.preamble_symbols(ft)
    x = rng.standard_normal(1500).astype(np.float32)
    x[rng.integers(0, len(x), 200)] = 0.0           # exact zeros count as positive
    x[100:100 + len(pre)] = 3.0 * pre               # a preamble,
    x[700:700 + len(pre)] = -0.5 * pre              # an inverted one,
    x[len(x) - len(pre):] = pre                     # and one in the last full window
    x[300:300 + len(pre)] = np.where(pre > 0, 0.0, -1.0)  # a preamble whose positive symbols are exact zeros
    dec = TelemetryDecoder(1, "full", gpu)
    for n in (len(x), 1025, 257, 256, len(pre) + 1, len(pre), len(pre) - 1, 1):   # several blocks, a block boundary, and blocks shorter than the preamble
        block = x[len(x) - n:]
        got = dec.preamble_scan(ft, block)
        assert got.dtype == np.int8 and np.array_equal(got, R.preamble_corr(block, ft)), n
    full = dec.preamble_scan(ft, x)
    assert full[100] == len(pre) and full[700] == -len(pre) and full[300] == len(pre) and full[len(x) - len(pre)] == len(pre)
    assert np.array_equal(dec.preamble_scan(ft, -np.zeros(40, np.float32)), R.preamble_corr(np.zeros(40, np.float32), ft))  # -0.0 is not < 0 either
    dec.close()


@pytest.mark.parametrize("ft", [1, 2, 3])
def test_frame_sync_returns_the_transmitted_pages_and_the_180_degree_flag(gpu, ft):
    symbols, expected = cases.three_page_case(ft)
    for sign, inverted in ((1.0, False), (-1.0, True)):
        fs = GalileoFrameSync(ft, 2, device=gpu)
        pages = fs.push({1: sign * symbols[:len(symbols) // 2]}) + fs.push({1: sign * symbols[len(symbols) // 2:]})
        cases.check_pages(pages, expected, inverted)
        assert all(p.channel == 1 for p in pages) and fs.state(1) == 2
        fs.close()
