"""CPU reference of the joint GP posterior and of the sampler's random stream (test infrastructure; numpy, products in np.longdouble).

What gabo_gp_posterior_joint computes (csrc/gp_posterior.hip): V = os k* linv^T over the lower triangle of linv, Sigma = os k** - V V^T from the
lower triangle of k**, mean = mean + os k* alpha - here in extended precision, next to the entrywise running-error bounds the GPU tests assert:
a dot product of length n evaluated in any order in fp64 is off by at most n u sum|a_i b_i| (u = 2^-53; Higham, Accuracy and Stability, ch. 3),
and Sigma chains two of them behind one more product and one subtraction: the tests assert (2 n + 8) u S with
S = os |k**| + Vabs Vabs^T, Vabs = os |k*| |linv|^T - n u per dot product and 8 u for the scaling, the subtraction and the reference's own
rounding to fp64.  (The strict worst case is larger by n u, the rounded V entering both factors of the second product; the tests keep the
tighter figure.)  The sampler's normals restate Philox.normal2 of csrc/gabo_philox.hpp on
oracle.selection.philox4x32_10 (item = sample, draw k -> coordinates 2k and 2k + 1, tag "mvnz")."""
import numpy as np

from oracle import selection as osel

U = 2.0 ** -53
MVN_TAG = 0x6D766E7A
LADDER = (0.0, 1e-8, 1e-7, 1e-6)


def _ld(a):
    return np.asarray(a, dtype=np.longdouble)


def joint_reference(kstar, kss, linv, alpha, mean, outputscale):
    """-> dict(mean, cov: float64 roundings of the extended-precision results; mean_scale, cov_scale: the S of the bounds above)"""
    ks, li = _ld(kstar), np.tril(_ld(linv))
    kl = np.tril(_ld(kss))
    kfull = kl + np.tril(kl, -1).T                              # what the lower triangle says
    osl = np.longdouble(outputscale)
    v = osl * (ks @ li.T)
    cov = osl * kfull - v @ v.T
    mu = np.longdouble(mean) + osl * (ks @ _ld(alpha))
    vabs = osl * (np.abs(ks) @ np.abs(li).T)
    return {"mean": mu.astype(np.float64), "cov": cov.astype(np.float64),
            "mean_scale": (abs(np.longdouble(mean)) + osl * (np.abs(ks) @ np.abs(_ld(alpha)))).astype(np.float64),
            "cov_scale": (osl * np.abs(kfull) + vabs @ vabs.T).astype(np.float64)}


def random_joint_case(m, n, seed):
    """random k* (m x n), a random symmetric k** (m x m), linv from a random SPD matrix, alpha: the inputs of one covariance launch"""
    rng = np.random.default_rng(seed)
    kstar = rng.uniform(-1.0, 1.0, (m, n))
    a = rng.uniform(-1.0, 1.0, (m, m))
    kss = 0.5 * (a + a.T)
    b = rng.standard_normal((n, n + 3))
    ky = b @ b.T / n + 0.5 * np.eye(n)
    linv = np.linalg.inv(np.linalg.cholesky(ky))
    linv = np.tril(linv)
    alpha = rng.standard_normal(n)
    return kstar, kss, linv, alpha, 0.37, 1.9


def mvn_normals(seed, samples, m):
    """samples x m standard normals as mvn_sample_kernel / mvn_base_samples_kernel draw them (agreement to the rounding of log / sincospi / sqrt)"""
    idx = np.arange(samples, dtype=np.uint64)
    out = np.empty((samples, m), dtype=np.float64)
    key = [np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF)]
    for k in range((m + 1) // 2):
        ctr = np.stack([(idx & np.uint64(0xFFFFFFFF)).astype(np.uint32), (idx >> np.uint64(32)).astype(np.uint32),
                        np.full(samples, k, dtype=np.uint32), np.full(samples, MVN_TAG, dtype=np.uint32)], axis=-1)
        o = osel.philox4x32_10(ctr, key)
        a = ((o[:, 0].astype(np.uint64) << np.uint64(32)) | o[:, 1].astype(np.uint64)) >> np.uint64(11)
        b = ((o[:, 2].astype(np.uint64) << np.uint64(32)) | o[:, 3].astype(np.uint64)) >> np.uint64(11)
        u1 = (a.astype(np.float64) + 1.0) * 2.0 ** -53
        u2 = b.astype(np.float64) * 2.0 ** -53
        r = np.sqrt(-2.0 * np.log(u1))
        out[:, 2 * k] = r * np.cos(2.0 * np.pi * u2)
        if 2 * k + 1 < m:
            out[:, 2 * k + 1] = r * np.sin(2.0 * np.pi * u2)
    return out


def gaussian_posterior(d_train, d_star, d_ss, y, beta, outputscale, noise, mean):
    """oracle.gp-style posterior of the latent f from DISTANCE matrices and a Gaussian kernel exp(-beta d^2): -> (mean, cov, cond(Ky))"""
    ky = outputscale * np.exp(-beta * d_train ** 2) + noise * np.eye(len(y))
    ks = outputscale * np.exp(-beta * d_star ** 2)
    kss = outputscale * np.exp(-beta * d_ss ** 2)
    sol = np.linalg.solve(ky, np.concatenate([ks.T, (np.asarray(y) - mean)[:, None]], axis=1))
    return mean + ks @ sol[:, -1], kss - ks @ sol[:, :-1], np.linalg.cond(ky)


def cholesky_residual_ok(L, a):
    """|L L^T - a| <= 2 (m + 1) u |L| |L|^T entrywise (the backward-error bound of Cholesky, Higham Thm 10.3, doubled) -> (ok, worst ratio)"""
    m = a.shape[0]
    Ll = _ld(L)
    res = np.abs(Ll @ Ll.T - _ld(a))
    bound = 2 * (m + 1) * U * (np.abs(Ll) @ np.abs(Ll).T)
    ratio = float(np.max(res / bound))
    return bool(np.all(res <= bound)), ratio
