"""The cases on which the device SPD sampler (gabotorch_amd/csrc/spd_sample.hip) is compared with its oracle (oracle.selection.spd_samples), shared
by the oracle's own CPU tests (tests/test_oracle_selection.py) and the device tests (tests/test_gpu_spd_sampler.py); each oracle run is computed
once per process and handed out read-only.

The per-sample bound of the comparison, |X_dev - X_oracle|_max <= 16 d eps kappa_i max_eig:
  * the device's normals differ from the correctly rounded ones by a few ulp (log, sincospi, their product);
  * Gram-Schmidt passes a relative perturbation delta of a column on to Q as at most about c delta kappa, kappa = max_c |g_c| / |r_c|;
  * X = Q diag(lam) Q^T moves by at most 2 max_eig |dQ|;
  * together about 10 d eps kappa max_eig; 16 is the margin.
The oracle has to meet a quarter of it when run in plain double with numpy's libm (tests/test_oracle_selection.py)."""
import functools

import numpy as np

from oracle import selection as osel

EPS = float(np.finfo(np.float64).eps)
N = 130                                     # three blocks of 64 lanes, the last one with 2
LO, HI = 0.3, 4.0
SEEDS = (1234, 0x9E3779B97F4A7C15)
ORDERS = tuple(range(1, 17))                # 1 ... 8: the register instantiations; 9 ... 16: the LDS form
FIRST_HIGH = 2 ** 32 - 3                    # eight samples from here straddle the counter's low word
# (seed, first, count, d): every order under both seeds, the counter's high word, the key's high word and top bit
CASES = tuple((s, 0, N, d) for s in SEEDS for d in ORDERS) \
    + tuple((SEEDS[1], FIRST_HIGH, 8, d) for d in (3, 10)) \
    + tuple((s, 0, N, d) for s in (0, 2 ** 64 - 1, 1 << 32) for d in (4, 11))


def bound(d, kappa, max_eig=HI):
    return 16.0 * d * EPS * np.asarray(kappa) * max_eig


def spectrum_bound(d, max_eig=HI):
    return 64.0 * d * EPS * max_eig


@functools.lru_cache(maxsize=None)
def oracle(seed, first, count, d, min_eig=LO, max_eig=HI, work=np.longdouble):
    out = osel.spd_samples(seed, first, count, d, min_eig, max_eig, work=work)
    for a in out:
        a.setflags(write=False)
    return out
