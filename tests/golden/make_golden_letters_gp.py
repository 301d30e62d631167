#!/usr/bin/env python3
"""The GP-regression problem of the reference's SPD demo as a fixture (development container only; it imports the reference and reads its data).

    python -W ignore tests/golden/make_golden_letters_gp.py

examples/kernels/spd/spd_kernels.py:85-137, restated without the plots: the first demonstration of data/2Dletters/C.mat (200 positions, time =
index), every position p turned into the SPD matrix Expmap_I(0.01 p p^T) by the reference's own expmap and symmetric_matrix_to_vector_mandel
(spd_utils.py:104-120, :57-76); every second point is a test point (100 of them, the whole letter), and the training set is those 100 minus
id_to_remove of :115 (79 points).  Stored next to the points: the reference's affine_invariant_distance_torch (spd_utils_torch.py:53-120) between
them - train x train, test x train, test x test - and the FIXED hyper-parameters the tests and examples/spd_kernels.py predict with (the demo fits
its own; a fit is not what this fixture is about).  Output: tests/golden/letters_gp.npz (arrays only).

The only shim is `torch.symeig` (removed from torch >= 1.13; the reference calls it at spd_utils_torch.py:110), mapped onto
`torch.linalg.eigh(UPLO='U')`, which is what symeig(upper=True) computed - as tests/golden/make_golden.py does.  The distances are taken
with torch's default dtype set to float64: the reference collects the eigenvalues in a torch.zeros(...) of the default dtype (:108), which in
float32 leaves 2e-7 of noise on a distance - enough to make the posterior covariance of this problem indefinite by 1e-3.  (The reference adds
1e-15 under the square root, :120: its self-distances are 3.2e-8, stored as they come.)"""
import collections
import os
import sys

import numpy as np
import torch
from scipy.io import loadmat

REF = os.environ.get("GABO_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)

_R = collections.namedtuple("symeig", ["eigenvalues", "eigenvectors"])
torch.symeig = lambda A, eigenvectors=False, upper=True: _R(*torch.linalg.eigh(A, UPLO="U" if upper else "L"))

from BoManifolds.Riemannian_utils.spd_utils import expmap, symmetric_matrix_to_vector_mandel, vector_to_symmetric_matrix_mandel  # noqa: E402
from BoManifolds.Riemannian_utils.spd_utils_torch import affine_invariant_distance_torch  # noqa: E402


def real(a):
    a = np.asarray(a)
    return np.ascontiguousarray(a.real if np.iscomplexobj(a) else a, dtype=np.float64)


def main():
    torch.set_default_dtype(torch.float64)
    data_demos = loadmat(os.path.join(REF, "data", "2Dletters", "C.mat"))["demos"][0]
    pos = data_demos[0]["pos"][0][0]                                     # 2 x 200 (nb_samples = 1: the first demonstration)
    time = np.arange(pos.shape[1]) * 1.0
    mandel = np.stack([real(symmetric_matrix_to_vector_mandel(expmap(0.01 * np.dot(pos[:, n][:, None], pos[:, n][None]), np.eye(2))))
                       for n in range(pos.shape[1])])                    # 200 x 3
    x_test, y_test = mandel[::2], time[::2]                              # :130-134
    id_to_remove = np.hstack((np.arange(24, 37), np.arange(68, 76)))     # :115
    train_idx = np.delete(np.arange(x_test.shape[0]), id_to_remove)
    x_train, y_train = x_test[train_idx], y_test[train_idx]

    def mats(v):
        return torch.tensor(np.stack([vector_to_symmetric_matrix_mandel(r) for r in v]))

    mt, mr = mats(x_test), mats(x_train)
    out = {
        "x_test": x_test, "y_test": y_test, "train_idx": train_idx.astype(np.int64), "y_train": y_train,
        "dist_train_train": real(affine_invariant_distance_torch(mr, mr).numpy()),
        "dist_test_train": real(affine_invariant_distance_torch(mt, mr).numpy()),
        "dist_test_test": real(affine_invariant_distance_torch(mt, mt).numpy()),
        "beta": np.float64(1.3), "outputscale": np.float64(2000.0), "noise": np.float64(2.0), "mean": np.float64(0.0),
    }
    path = os.path.join(HERE, "letters_gp.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes; n = {len(train_idx)}, m = {len(x_test)}, max distance {out['dist_test_test'].max():.3f}")


if __name__ == "__main__":
    main()
