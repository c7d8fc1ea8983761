"""CPU: the stage-by-stage reference of tests/ntt_ref.py, proved against oracle.pyref.poly before any GPU result is compared
with it.  The passes of the default plan (tests/host_shim/ntt_plan_driver.cpp) are chained as DIF then bitrev and as bitrev
then DIT; both must give Domain.fft / ifft, and with the epilogue coset_fft / coset_ifft."""
import random

import pytest

from oracle.pyref.params import CURVES
from oracle.pyref.poly import Domain
from tests import ntt_plan
from tests import ntt_ref as nr

CURVE_NAMES = ["bn254", "bls12_381"]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    return ntt_plan.load(tmp_path_factory.mktemp("ntt_plan"))[1]


def chain(cp, x, logn, ps, dit, inverse):
    for lo, nst, _ in (ps if dit else ps[::-1]):
        x = nr.pass_ref(cp, x, logn, lo, nst, dit, inverse)
    return x


def dif(cp, x, logn, ps, inverse):
    return nr.bitrev(chain(cp, x, logn, ps, 0, inverse))


def dit(cp, x, logn, ps, inverse):
    return chain(cp, nr.bitrev(x), logn, ps, 1, inverse)


def test_bitrev():
    assert nr.bitrev([0]) == [0] and nr.bitrev([0, 1]) == [0, 1]
    assert nr.bitrev(list(range(8))) == [0, 4, 2, 6, 1, 5, 3, 7]
    x = list(range(64))
    assert nr.bitrev(nr.bitrev(x)) == x


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_tables(cname):
    cp = CURVES[cname]
    for inverse in (0, 1):
        t = nr.stage_tables(cp, 5, inverse)
        w = nr.root(cp, 5, inverse)
        for s in range(5):
            for j in range(1 << s):
                assert t[(1 << s) - 1 + j] == pow(w, j << (4 - s), cp.r)
        assert nr.squarings(cp, 5, inverse) == [pow(w, 1 << k, cp.r) for k in range(5)]
        g = pow(cp.fr_generator, -1, cp.r) if inverse else cp.fr_generator
        pw = nr.pow_tables(cp, inverse)
        assert len(pw) == 3 * 2048
        for j in (0, 1, 2047, 2048, 2049, 4095, 4096, 6143):
            assert pw[j] == pow(g, (j & 2047) << (11 * (j >> 11)), cp.r)


@pytest.mark.parametrize("log_m", range(1, 11))
@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_chained_passes_are_the_oracle_transforms(plans, cname, log_m):
    cp = CURVES[cname]
    r, g = cp.r, cp.fr_generator
    ginv = pow(g, -1, r)
    rng = random.Random(1000 * cp.cid + log_m)
    m = 1 << log_m
    x = [rng.randrange(r) for _ in range(m)]
    x[0], x[-1] = r - 1, 0
    _, ps = plans[log_m, ntt_plan.DEFAULT_TILE_LOG, ntt_plan.DEFAULT_UPPER_MAX]
    assert sum(nst for _, nst, _ in ps) == log_m
    D = Domain(cp, m)
    minv = pow(m, -1, r)
    fft, ifft = D.fft(x), D.ifft(x)
    assert dif(cp, x, log_m, ps, 0) == fft
    assert dit(cp, x, log_m, ps, 0) == fft
    assert [v * minv % r for v in dif(cp, x, log_m, ps, 1)] == ifft
    assert [v * minv % r for v in dit(cp, x, log_m, ps, 1)] == ifft
    # coset fft: coefficient j times g^j, then the transform.  A natural-order vector is the bit-reversed order of its own
    # bit-reversal, so the epilogue's g^bitrev(i) applied to bitrev(x) scales x[j] by g^j
    pre = nr.bitrev(nr.epilogue_ref(cp, nr.bitrev(x), log_m, 2, None, g, None, None))
    assert pre == [v * pow(g, j, r) % r for j, v in enumerate(x)]
    assert dif(cp, pre, log_m, ps, 0) == D.coset_fft(x, g)
    assert dit(cp, pre, log_m, ps, 0) == D.coset_fft(x, g)
    # coset ifft as hk_ntt runs it: DIF with w^-1, epilogue post = 3 (g^-bitrev(i), then 1/m) on the bit-reversed result
    y = nr.epilogue_ref(cp, chain(cp, x, log_m, ps, 0, 1), log_m, 3, minv, ginv, None, None)
    assert nr.bitrev(y) == D.coset_ifft(x, g)
    y = nr.epilogue_ref(cp, nr.bitrev(dit(cp, x, log_m, ps, 1)), log_m, 3, minv, ginv, None, None)
    assert nr.bitrev(y) == D.coset_ifft(x, g)
    # the subtraction step sits between the two: (v g^-j - sub kc) / m
    sub = [rng.randrange(r) for _ in range(m)]
    kc = rng.randrange(1, r)
    z = nr.epilogue_ref(cp, chain(cp, x, log_m, ps, 0, 1), log_m, 7, minv, ginv, sub, kc)
    want = [(c * m - s * kc) * minv % r for c, s in zip(D.coset_ifft(x, g), nr.bitrev(sub))]
    assert nr.bitrev(z) == want
