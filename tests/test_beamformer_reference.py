"""CPU tests of the checker of the antenna-array front end: tests/beamformer_reference.py against the reference block's own output
(tests/golden/beamformer.npz), its power to see a kernel the compiler contracted, the weight helpers of gnss_sdr_amd.array against numpy.linalg, and
the end-to-end scenario of tests/test_beamformer_gpu.py worked through on the CPU."""
import os

import numpy as np
import pytest

import beamformer_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beamformer.npz")


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def test_restatement_at_default_weights_equals_the_block_bit_for_bit():
    with np.load(GOLDEN) as z:
        x, y = z["x"], z["y"]
    assert x.shape == (8, 4099, 2) and y.shape == (4099, 2) and x.dtype == y.dtype == np.float32
    mag = np.abs(x[x != 0])
    assert np.log2(mag.max() / mag.min()) > 40          # many binades
    re, im = R.items_to_complex(x)
    got = R.beamform(re, im, np.ones((1, 8), np.complex64))[0]
    assert np.array_equal(_bits(got), _bits(y).reshape(-1))


def test_restatement_follows_item_order_and_conjugation():
    items = np.array([[[3, -4], [0, 5]]], np.int8)
    re, im = R.items_to_complex(items)
    assert re.tolist() == [[3.0, 0.0]] and im.tolist() == [[-4.0, 5.0]]
    re, im = R.items_to_complex(items, first_is_q=True, inverted_spectrum=True)
    assert re.tolist() == [[-4.0, 5.0]] and im.tolist() == [[-3.0, -0.0]] and np.signbit(im[0, 1])
    # (0, 0) + a product of -0 is +0, as in the block
    out = R.beamform(np.array([[-0.0]], np.float32), np.array([[0.0]], np.float32), np.array([[1.0]], np.complex64))
    assert not np.signbit(out.real[0, 0])


@pytest.mark.parametrize("item_type", ["gr_complex", "ishort", "ibyte"])
def test_a_contracted_kernel_would_change_the_gpu_cases(item_type):
    """the GPU test compares bit for bit with beamform(); for every item type and antenna count of its grid a fused multiply-add changes outputs"""
    for A in (1, 2, 3, 8):
        re, im = R.items_to_complex(R.case_items(item_type, A))
        for B in (1, 3, 8):
            w = R.case_weights(B, A)
            plain, fused = R.beamform(re, im, w), R.beamform(re, im, w, contracted=True)
            changed = int(np.count_nonzero(_bits(plain) != _bits(fused)))
            assert changed > 0, (item_type, A, B)
            assert np.all(np.isfinite(plain.view(np.float32)))


def test_power_inversion_weights_satisfy_their_definition():
    from gnss_sdr_amd.array import power_inversion_weights
    rng = np.random.default_rng(3)
    for A, ref, loading in ((2, 0, 0.0), (4, 0, 0.0), (4, 2, 0.5), (8, 7, 1e-3)):
        X = rng.standard_normal((A, 5 * A)) + 1j * rng.standard_normal((A, 5 * A))
        Rm = X @ X.conj().T
        w = power_inversion_weights(Rm, reference=ref, loading=loading)
        assert w.dtype == np.complex64 and w.shape == (A,)
        Rl = Rm + loading * np.eye(A)
        e = np.zeros(A)
        e[ref] = 1.0
        v = np.linalg.inv(Rl) @ e
        v = v / (e @ v)
        np.testing.assert_allclose(w, np.conj(v), rtol=2e-6, atol=0)
        assert w[ref] == 1.0
        # the minimiser of v^H R v under v[ref] = 1: the gradient R v is parallel to e
        g = Rl @ np.conj(w.astype(np.complex128))
        assert np.all(np.abs(np.delete(g, ref)) <= 1e-5 * np.abs(g[ref]))
    # the scale of R cancels
    np.testing.assert_allclose(power_inversion_weights(Rm), power_inversion_weights(Rm / 123.0), rtol=1e-6)


def test_mvdr_weights_satisfy_their_definition():
    from gnss_sdr_amd.array import mvdr_weights
    rng = np.random.default_rng(4)
    for A, loading in ((3, 0.0), (4, 0.25), (8, 0.0)):
        X = rng.standard_normal((A, 6 * A)) + 1j * rng.standard_normal((A, 6 * A))
        Rm = X @ X.conj().T
        s = R.steering(A, 25.0)
        w = mvdr_weights(Rm, s, loading=loading)
        assert w.dtype == np.complex64 and w.shape == (A,)
        Rl = Rm + loading * np.eye(A)
        Ri = np.linalg.inv(Rl)
        v = Ri @ s / (s.conj() @ Ri @ s)
        np.testing.assert_allclose(w, np.conj(v), rtol=5e-6, atol=1e-7)
        # distortionless: the block's output for x = s is sum_a s_a w_a = v^H s = 1
        assert abs(np.sum(s * w.astype(np.complex128)) - 1.0) < 1e-6
        # least output power among distortionless weights: any feasible perturbation costs power
        v0 = np.conj(w.astype(np.complex128))
        d = rng.standard_normal(A) + 1j * rng.standard_normal(A)
        d -= s * (s.conj() @ d) / (s.conj() @ s)          # d^H s = 0
        p0 = (v0.conj() @ Rl @ v0).real
        assert ((v0 + 0.1 * d).conj() @ Rl @ (v0 + 0.1 * d)).real > p0


def test_end_to_end_scenario_on_the_cpu():
    """what tests/test_beamformer_gpu.py::test_end_to_end asks of the GPU, with the restatement and the PCPS oracle: antenna 0 alone does not acquire
    the jammed satellite, the power-inversion beam does, at the right delay and Doppler -- also at jammer amplitudes 3 and 30"""
    import oracle
    from gnss_sdr_amd.array import power_inversion_weights
    from oracle.pcps_oracle import PcpsOracle, compute_threshold
    thr = compute_threshold(R.E2E_PFA, 4000, 40, 1)
    assert thr == pytest.approx(44.05, abs=0.01)
    ora = PcpsOracle(**R.E2E_ACQ)
    ora.set_local_code(oracle.ca_code_complex_sampled(R.E2E["prn"], R.E2E["fs"]))
    for amp in (10.0, 3.0, 30.0):
        x = R.e2e_block(jammer_amplitude=amp)
        re, im = x.real.copy(), x.imag.copy()
        w = power_inversion_weights(R.covariance(re, im))
        beams = R.beamform(re, im, np.stack([w, np.eye(4, dtype=np.complex64)[0]]))
        assert np.array_equal(_bits(beams[1]), _bits(x[0] + np.complex64(0)))
        beam, ant0 = ora.dwell(beams[0]), ora.dwell(beams[1])
        print(f"jammer amplitude {amp}: antenna 0 statistic {ant0['test_statistics']:.2f}, beam {beam['test_statistics']:.1f} at "
              f"({beam['index_time']}, {beam['doppler_hz']} Hz), threshold {thr:.2f}")
        assert ant0["test_statistics"] < thr
        assert beam["test_statistics"] > 2.0 * thr
        assert (beam["index_time"], beam["doppler_hz"]) == (2826, 1250)
