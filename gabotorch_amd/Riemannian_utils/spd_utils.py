"""numpy-facing SPD helpers with the reference's names and argument order (BoManifolds/Riemannian_utils/spd_utils.py).
The Mandel maps and `spd_sample` are host numpy (they feed host callbacks and a host RNG: SURVEY 8b); the exp/log maps and
the distance go through the HIP manifold kernels."""
import numpy as np
import torch

from .. import _lib, ops


def _mandel_index(d):
    r, c = [], []
    for k in range(d):
        for i in range(d - k):
            r.append(i)
            c.append(i + k)
    return np.array(r), np.array(c)


def symmetric_matrix_to_vector_mandel(M):
    """(spd_utils.py:57-76)"""
    M = np.asarray(M)
    r, c = _mandel_index(M.shape[-1])
    return M[..., r, c] * np.where(r == c, 1.0, 2.0 ** 0.5)


def vector_to_symmetric_matrix_mandel(v):
    """(spd_utils.py:79-101)"""
    v = np.asarray(v, dtype=float)
    d = int((-1.0 + (1.0 + 8.0 * v.shape[-1]) ** 0.5) / 2.0)
    r, c = _mandel_index(d)
    s = np.where(r == c, 1.0, 1.0 / 2.0 ** 0.5)
    M = np.zeros(v.shape[:-1] + (d, d))
    M[..., r, c] = v * s
    M[..., c, r] = v * s
    return M


def expmap(U, S):
    """Exp_S(U)   (spd_utils.py:104-120; tangent first, base second)"""
    return ops.spd_manifold_op(_lib.GABO_SPD_EXP, torch.as_tensor(np.asarray(S)), torch.as_tensor(np.asarray(U))).numpy()


def logmap(X, S):
    """Log_S(X)   (spd_utils.py:123-139; point first, base second)"""
    return ops.spd_manifold_op(_lib.GABO_SPD_LOG, torch.as_tensor(np.asarray(S)), torch.as_tensor(np.asarray(X))).numpy()


def affine_invariant_distance(S1, S2):
    """(spd_utils.py:180-197)"""
    return float(ops.spd_manifold_op(_lib.GABO_SPD_DIST, torch.as_tensor(np.asarray(S1)), torch.as_tensor(np.asarray(S2))))


def spd_sample(self):
    """Random SPD matrix with eigenvalues U[self.min_eig, self.max_eig]; numpy GLOBAL RNG, the reference's draw order
    (spd_utils.py:290-306).  Meant to be bound as `manifold.rand` (examples/gabo_spd.py:102)."""
    d = self.min_eig * np.ones(1) + (self.max_eig - self.min_eig) * np.random.rand(self._n)
    u, _ = np.linalg.qr(np.random.randn(self._n, self._n))
    return np.dot(u, np.dot(np.diag(d), u.T))


def parallel_transport_operator(S1, S2):
    """(S2 S1^-1)^(1/2)   (spd_utils.py:200-213), as L1 sqrtm(L1^-1 S2 L1^-T) L1^-1 with L1 = chol(S1): S2 S1^-1 is similar, through L1, to the SPD matrix
    in the middle, whose square root is one GABO_SPD_SQRTM launch.  Real by construction (the reference's fractional_matrix_power may hand back a
    complex dtype with zero imaginary part).  P S1 P^T = S2."""
    S1, S2 = np.asarray(S1, dtype=float), np.asarray(S2, dtype=float)
    L = np.linalg.cholesky(S1)
    Li = np.linalg.inv(L)
    M = Li @ S2 @ Li.T
    R = ops.spd_manifold_op(_lib.GABO_SPD_SQRTM, torch.as_tensor(0.5 * (M + M.T))).numpy()
    return L @ R @ Li


def parallel_transport_operator_mandel_vector(s1, s2):
    """(spd_utils.py:216-232)"""
    return parallel_transport_operator(vector_to_symmetric_matrix_mandel(s1), vector_to_symmetric_matrix_mandel(s2))


def mean(data, nb_iter=10):
    """Frechet mean of the N x d x d SPD matrices `data`, started at data[0]   (spd_utils.py:235-259): one enqueued chain of launches
    (ops.spd_frechet_mean) instead of 2 N nb_iter host eigen-decompositions."""
    data = np.asarray(data, dtype=float)
    return vector_to_symmetric_matrix_mandel(ops.spd_frechet_mean(torch.as_tensor(symmetric_matrix_to_vector_mandel(data)), iters=nb_iter).numpy())


def mean_mandel_vector(data, nb_iter=10):
    """The same for Mandel vectors in the COLUMNS of `data` (d_vec x N) -> (d_vec,)   (spd_utils.py:262-287)"""
    data = np.asarray(data, dtype=float)
    return ops.spd_frechet_mean(torch.as_tensor(np.ascontiguousarray(data.T)), iters=nb_iter).numpy()
