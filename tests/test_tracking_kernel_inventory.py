"""Which E/P/L correlator kernels the library holds (csrc/mcorr_kernels.h, instantiated by csrc/multicorrelator.hip at 256 threads and by
csrc/multicorrelator_t128.hip at 128), read from the built library's code-object metadata (no GPU needed; method of tests/test_kernel_resources.py).

The four-wave unit builds every flavour its launcher can pick.  The two-wave unit builds only what mcorr_launch_epl_t128 can launch -- use_128() admits the
standard mode without fused jobs and without a code window, two or three taps -- i.e. three flavours of mcorr_kernel_t128<3, 0, ...> and the walk.  Both sets
are spelled out: a flavour that becomes reachable is added here on purpose, and one that is instantiated without a launch site shows up as a difference."""
import os
import re

import pytest

import gnss_sdr_amd
from kernel_metadata import kernels

# mcorr_kernel<NT, MODE, AUX, RUNS, WIN, PAIR, HALF>
FLAVOUR = re.compile(r"mcorr_kernel(_t128)?ILi(\d)ELi(\d)ELb([01])ELb([01])ELb([01])ELb([01])ELb([01])EE")

FOUR_WAVE = (
    # every tap class: whole code and code window in the standard mode, the two high-dynamics modes
    {(nt, 0, 0, 0, 0, 0, 0) for nt in (1, 3, 5, 8)} | {(nt, 0, 0, 0, 1, 0, 0) for nt in (1, 3, 5, 8)}
    | {(nt, 1, 0, 0, 0, 0, 0) for nt in (1, 3, 5, 8)} | {(nt, 2, 0, 0, 0, 0, 0) for nt in (1, 3, 5, 8)}
    # fused jobs: the 3- and 5-tap kernels, whole code and code window
    | {(nt, 0, 1, 0, win, 0, 0) for nt in (3, 5) for win in (0, 1)}
    # E/P/L: paired taps (whole code, code window), half-chip taps
    | {(3, 0, 0, 0, 0, 1, 0), (3, 0, 0, 0, 1, 1, 0), (3, 0, 0, 0, 0, 1, 1)}
)
TWO_WAVE = {
    (3, 0, 0, 0, 0, 0, 0),  # per-tap trips (a launch that is not pair-eligible, or GSH_MC_PACKED_BODY=3)
    (3, 0, 0, 0, 0, 1, 0),  # paired taps
    (3, 0, 0, 0, 0, 1, 1),  # half-chip taps: the headline kernel
}


@pytest.fixture(scope="module")
def names():
    lib = gnss_sdr_amd._lib.LIB_PATH
    if not os.path.exists(lib):
        pytest.skip("library not built")
    k = kernels(lib)
    assert len(k) > 50, "no gfx950 code objects found in the library"
    return sorted(k)


def _flavours(names, t128):
    found = [tuple(int(g) for g in m.groups()[1:]) for m in map(FLAVOUR.search, names) if m and bool(m.group(1)) == t128]
    assert len(found) == len(set(found)), found  # each flavour in one translation unit only
    return set(found)


def test_the_expected_sets_are_what_the_docstring_says():
    assert len(FOUR_WAVE) == 23 and len(TWO_WAVE) == 3 and TWO_WAVE <= FOUR_WAVE


def test_the_four_wave_unit_holds_every_flavour_and_the_reduction(names):
    got = _flavours(names, t128=False)
    assert got == FOUR_WAVE, (sorted(got - FOUR_WAVE), sorted(FOUR_WAVE - got))
    assert len([n for n in names if "mcorr_reduce_partials" in n]) == 1, [n for n in names if "mcorr_reduce_partials" in n]


def test_the_two_wave_unit_holds_the_three_reachable_flavours_and_the_walk(names):
    got = _flavours(names, t128=True)
    assert got == TWO_WAVE, (sorted(got - TWO_WAVE), sorted(TWO_WAVE - got))
    assert len([n for n in names if "mcorr_walk_kernel_t128" in n]) == 1
    # nothing else of the correlator bank at 128 threads: the three flavours, the walk
    assert len([n for n in names if "mcorr_" in n and "_t128" in n]) == 4, [n for n in names if "mcorr_" in n and "_t128" in n]
    assert not [n for n in names if "mcorr_reduce_partials_t128" in n]
