"""Synthetic symbol streams for the frame synchroniser tests (CPU: tests/test_tlm_frame_sync.py on the numpy engine; GPU: tests/test_tlm_gpu.py on the
device), built with the encoder of tests/tlm_reference.py.  A stream is pages back to back, each a preamble and a coded page, then `required` symbols of
+1 (no preamble correlates with a constant), so that the window of the last page's position completes and no position after it does."""
import numpy as np

import tlm_reference as R


def pad(frame_type):
    return np.ones(R.GEOMETRY[frame_type]["required"], np.float32)


def pages_for(frame_type, rng, n_words, good=True):
    """n_words F/NAV or C/NAV pages, or n_words I/NAV words as 2 * n_words parts (even, odd, even, ...)"""
    if frame_type == 1:
        return [part for _ in range(n_words) for part in R.inav_word(rng, good)]
    return [R.nav_page(rng, frame_type, good) for _ in range(n_words)]


def three_page_case(frame_type, seed=5):
    """-> (symbols, expected): two pages the synchroniser locks on (their preambles are one period apart; neither is decoded), then three pages (I/NAV:
    three words, six parts).  expected: (preamble_index, bits, crc_ok) per returned page.  The I/NAV verdict is a latch that starts false and is first
    set by the odd part of the first decoded even/odd pair: the first returned part, an even one, still carries false."""
    rng = np.random.default_rng(seed)
    head = pages_for(frame_type, rng, 1) if frame_type == 1 else pages_for(frame_type, rng, 2)
    body = pages_for(frame_type, rng, 3)
    period = R.GEOMETRY[frame_type]["period"]
    expected = [((2 + k) * period, p, not (frame_type == 1 and k == 0)) for k, p in enumerate(body)]
    return np.concatenate([R.stream(frame_type, head + body), pad(frame_type)]), expected


def check_pages(pages, expected, inverted):
    assert len(pages) == len(expected), (len(pages), len(expected))
    for got, (index, bits, ok) in zip(pages, expected):
        assert got.preamble_index == index and got.inverted == inverted and got.crc_ok == ok, (got.preamble_index, index, got.inverted, got.crc_ok, ok)
        assert np.array_equal(got.bits, bits), index
