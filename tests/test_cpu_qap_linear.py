"""The identity behind the linear QAP chain (csrc/ntt.hip ntt_qap_linear), on the Python field reference:
H = icoset((a' b' - c') / Z) with a', b', c' the coset evaluations (three round trips) equals
(icoset(a' b') - ifft(c)) / Z, for every a, b, c; for c = a o b on the domain coefficient d - 1 is zero.
The linear form below is written as the device runs it: c's inverse transform unscaled, 1/d and 1/Z in one factor
of the epilogue."""
import pytest

import pyref
from pyref import GENERATOR, R, SplitMix64


def _three_round_trips(a, b, c, log_d):
    d = 1 << log_d
    a, b, c = (pyref.domain(pyref.domain(v, log_d, 1), log_d, 2) for v in (a, b, c))
    zinv = pow((pow(GENERATOR, d, R) - 1) % R, R - 2, R)
    return pyref.domain([((x * y - w) * zinv) % R for x, y, w in zip(a, b, c)], log_d, 3)


def _linear(a, b, c, log_d):
    d = 1 << log_d
    a, b = (pyref.domain(pyref.domain(v, log_d, 1), log_d, 2) for v in (a, b))
    winv = pow(pyref.omega(log_d), R - 2, R)
    c_raw = pyref.dft(c, winv)  # d * ifft(c)
    x = pyref.dft([(u * v) % R for u, v in zip(a, b)], winv)
    s = pow(d * (pow(GENERATOR, d, R) - 1) % R, R - 2, R)
    ginv = pow(GENERATOR, R - 2, R)
    return [((x[i] * pow(ginv, i, R) - c_raw[i]) * s) % R for i in range(d)]


@pytest.mark.parametrize("log_d", [3, 4])
def test_linear_form_equals_three_round_trips(log_d):
    d = 1 << log_d
    rng = SplitMix64(700 + log_d)
    a = [rng.fr() for _ in range(d)]
    b = [rng.fr() for _ in range(d)]
    sat = [(x * y) % R for x, y in zip(a, b)]
    h = _linear(a, b, sat, log_d)
    assert h == _three_round_trips(a, b, sat, log_d)
    assert h[d - 1] == 0 and any(h[:d - 1])
    c = [rng.fr() for _ in range(d)]
    h = _linear(a, b, c, log_d)
    assert h == _three_round_trips(a, b, c, log_d)
    assert h[d - 1] != 0
