"""Writes tests/golden/spd_ai_gauss_pin_d10.npz: the Gaussian-only launch of the SPD pairwise kernel at d = 10 on 9 x 70 points of the benchmark's
generator, inputs and output (the pin of tests/test_gpu_pairwise_occupancy.py).  Column NONPD_COL of x2 is symmetric, NaN-free and not positive
definite.  Needs an MI355X and the library whose bits are to be pinned (GABO_HIP_LIB selects another than the tree's):

    python tools/gen_spd_ai_gauss_pin.py [out.npz]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from tests.test_gpu_pairwise_gauss_finish import NONPD_COL, _mandel, _spd_from, synthetic_spd_mandel  # noqa: E402
from tests.test_gpu_pairwise_occupancy import D, PIN, PIN_N1, PIN_N2, gram  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", PIN)
    x1, x2 = synthetic_spd_mandel(PIN_N1, D, 4001), synthetic_spd_mandel(PIN_N2, D, 4002)
    rng = np.random.default_rng(4003)
    bad = rng.uniform(0.05, 5.0, size=(1, D))
    bad[0, D // 2] *= -1.0
    x2[NONPD_COL] = _mandel(_spd_from(rng, bad))[0]
    k = gram(x1, x2)
    assert k.shape == (PIN_N1, PIN_N2) and np.isnan(k[:, NONPD_COL]).all() and np.isfinite(np.delete(k, NONPD_COL, axis=1)).all()
    np.savez(out, x1=x1, x2=x2, k=k)
    print(f"{out}: x1 {x1.shape}, x2 {x2.shape}, k {k.shape}, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
