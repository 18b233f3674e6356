"""gnss_sdr_amd.telemetry.GalileoFrameSync (the frame synchroniser of galileo_telemetry_decoder_gs.cc:953-1110, restated on the host) on synthetic symbol
streams, with the numpy engine of tests/tlm_reference.py in place of the device (tests/test_tlm_gpu.py runs the same streams on the device)."""
import numpy as np
import pytest

import tlm_reference as R
import tlm_sync_cases as cases
from gnss_sdr_amd.telemetry import CRC_ERROR_LIMIT, FRAME, GalileoFrameSync, symbols_from_records

FRAME_TYPES = [1, 2, 3]


def _sync(frame_type, metric="full", n_channels=1):
    return GalileoFrameSync(frame_type, n_channels, metric=metric, engine=R.NumpyTelemetryDecoder(n_channels, metric))


def test_frame_table_agrees_with_the_restatement():
    for ft, g in R.GEOMETRY.items():
        f = FRAME[ft]
        assert (f["symbols"], f["info_bits"], f["preamble"], f["period"], f["required"]) == (g["symbols"], g["info_bits"], len(g["preamble"]), g["period"], g["required"])
        assert f["required"] == {1: 500, 2: 500, 3: 1000}[ft] + f["preamble"]  # d_required_symbols, galileo_telemetry_decoder_gs.cc:185, 204, 217


@pytest.mark.parametrize("frame_type", FRAME_TYPES)
def test_locks_after_two_preambles_one_period_apart_and_returns_the_pages(frame_type):
    symbols, expected = cases.three_page_case(frame_type)
    fs = _sync(frame_type)
    pages = fs.push({0: symbols})
    assert fs.state(0) == 2
    cases.check_pages(pages, expected, inverted=False)


@pytest.mark.parametrize("frame_type", FRAME_TYPES)
def test_pushing_symbol_by_symbol_blocks_gives_the_same_pages(frame_type):
    """the stream cut into uneven pushes (one of them a single symbol): what a push returns depends on the symbols so far, not on the cuts"""
    symbols, expected = cases.three_page_case(frame_type)
    fs = _sync(frame_type)
    cuts = [0, 1, 7, len(symbols) // 3, len(symbols) // 3 + 1, 2 * len(symbols) // 3, len(symbols)]
    pages = [p for a, b in zip(cuts, cuts[1:]) for p in fs.push({0: symbols[a:b]})]
    cases.check_pages(pages, expected, inverted=False)


@pytest.mark.parametrize("frame_type", FRAME_TYPES)
@pytest.mark.parametrize("shift", [-1, 1])
def test_no_lock_when_the_preambles_are_one_symbol_off_the_period(frame_type, shift):
    rng = np.random.default_rng(21)
    g = R.GEOMETRY[frame_type]
    first, second = cases.pages_for(frame_type, rng, 2)[:2]
    body = R.encode_page(first, frame_type)
    body = body[:-1] if shift < 0 else np.concatenate([body, [1.0]]).astype(np.float32)
    symbols = np.concatenate([R.preamble_symbols(frame_type), body, R.stream(frame_type, [second]), cases.pad(frame_type)])
    hits = np.nonzero(np.abs(R.preamble_corr(symbols, frame_type)) >= len(g["preamble"]))[0]
    assert list(hits) == [0, g["period"] + shift]  # the stream holds these two preambles and nothing that looks like one
    fs = _sync(frame_type)
    assert fs.push({0: symbols}) == []
    assert fs.state(0) == (1 if shift < 0 else 0)  # too early: still waiting; too late: start again (:1019-1022)


@pytest.mark.parametrize("frame_type", FRAME_TYPES)
def test_inverted_stream_gives_the_180_degree_flag_and_the_same_bits(frame_type):
    symbols, expected = cases.three_page_case(frame_type)
    fs = _sync(frame_type)
    cases.check_pages(fs.push({0: -symbols}), expected, inverted=True)


@pytest.mark.parametrize("frame_type", FRAME_TYPES)
def test_seven_consecutive_crc_failures_give_back_state_0(frame_type):
    rng = np.random.default_rng(31)
    head = cases.pages_for(frame_type, rng, 2)[:2]
    bad = (cases.pages_for(frame_type, rng, 4, good=False))[:CRC_ERROR_LIMIT + 1] if frame_type == 1 else cases.pages_for(frame_type, rng, CRC_ERROR_LIMIT + 1, good=False)
    period = R.GEOMETRY[frame_type]["period"]
    # six failures, then the window of the seventh page completes
    fs = _sync(frame_type)
    symbols = np.concatenate([R.stream(frame_type, head + bad), cases.pad(frame_type)])
    cut = len(symbols) - period
    pages = fs.push({0: symbols[:cut]})
    assert len(pages) == CRC_ERROR_LIMIT and not any(p.crc_ok for p in pages) and fs.state(0) == 2
    pages = fs.push({0: symbols[cut:]})
    assert len(pages) == 1 and not pages[0].crc_ok and fs.state(0) == 0
    # a good page after six failures clears the counter: six more failures do not lose the lock
    if frame_type != 1:
        good = cases.pages_for(frame_type, rng, 1)
        fs = _sync(frame_type)
        pages = fs.push({0: np.concatenate([R.stream(frame_type, head + bad[:6] + good + bad[:6]), cases.pad(frame_type)])})
        assert [p.crc_ok for p in pages] == [False] * 6 + [True] + [False] * 6 and fs.state(0) == 2


@pytest.mark.parametrize("frame_type", [2, 3])
def test_pages_after_the_loss_of_lock_are_dropped_and_the_search_resumes_there(frame_type):
    """one push holds the seven failing pages AND later good ones: the pages after the loss are not returned as a continuation; the synchroniser locks
    again on the next two preambles and returns what follows them"""
    rng = np.random.default_rng(41)
    head = cases.pages_for(frame_type, rng, 2)
    bad = cases.pages_for(frame_type, rng, CRC_ERROR_LIMIT + 1, good=False)
    tail = cases.pages_for(frame_type, rng, 4)
    period = R.GEOMETRY[frame_type]["period"]
    fs = _sync(frame_type)
    pages = fs.push({0: np.concatenate([R.stream(frame_type, head + bad + tail), cases.pad(frame_type)])})
    # positions: head 0, 1; bad 2..8 (lost at 8); tail 9..12: preambles 9 and 10 lock again, 11 and 12 are decoded
    assert [p.preamble_index // period for p in pages] == [2, 3, 4, 5, 6, 7, 8, 11, 12]
    assert [p.crc_ok for p in pages] == [False] * 7 + [True, True]
    assert np.array_equal(pages[-1].bits, tail[-1]) and fs.state(0) == 2


def test_inav_verdict_is_a_latch_that_changes_only_when_an_odd_part_follows_an_even_part():
    rng = np.random.default_rng(51)
    e0, o0 = R.inav_word(rng)
    e1, o1 = R.inav_word(rng)
    e2, o2 = R.inav_word(rng)
    e3, o3 = R.inav_word(rng)
    eb, ob = R.inav_word(rng, good=False)
    parts = [e0, o0,         # locked on, not decoded
             e1, o1,         # even-odd: the latch is set at the odd part
             o2,             # odd-odd: no even part is held, nothing changes (o2 would not match e1)
             e2, e3,         # even-even: nothing changes, e3 replaces e2
             o3,             # joins e3: stays true
             eb, ob,         # a failing pair clears it
             o1]             # an odd part alone does not set it again
    fs = _sync(1)
    pages = fs.push({0: np.concatenate([R.stream(1, parts), cases.pad(1)])})
    assert [p.crc_ok for p in pages] == [False, True, True, True, True, True, True, False, False]
    for p, want in zip(pages, parts[2:]):
        assert np.array_equal(p.bits, want)


def test_two_channels_in_one_push_and_the_reference_metric():
    a, exp_a = cases.three_page_case(2, seed=61)
    b, exp_b = cases.three_page_case(2, seed=62)
    for metric in ("full", "reference"):   # noise-free streams: the reference's decoder makes no error on them either
        fs = _sync(2, metric, n_channels=3)
        pages = fs.push({2: a, 0: -b})
        cases.check_pages([p for p in pages if p.channel == 2], exp_a, inverted=False)
        cases.check_pages([p for p in pages if p.channel == 0], exp_b, inverted=True)


def test_symbols_from_records_takes_the_flagged_epochs():
    from gnss_sdr_amd._lib import TrkEpoch
    recs = []
    for k in range(6):
        r = TrkEpoch()
        r.sample_counter, r.symbol_flags = 1000 * k, (1 if k % 2 else 2)
        r.p_data_accu[0], r.p_data_accu[1] = float(k) - 2.5, 9.0
        recs.append(r)
    sym, counters = symbols_from_records(recs)
    assert sym.dtype == np.float32 and list(sym) == [-1.5, 0.5, 2.5] and list(counters) == [1000, 3000, 5000]
