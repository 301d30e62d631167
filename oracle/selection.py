"""ORACLE (test infrastructure only - never imported by the product): the restart selection of an acquisition sweep as the device kernel
`sweep_select_kernel` (gabotorch_amd/csrc/spd_sweep.hip) performs it, restated in numpy.

What is restated: [3P] botorch.optim.initializers.initialize_q_batch_nonneg - the heuristic gen_batch_initial_conditions_manifold applies to
non-negative acquisition functions (BoManifolds/manifold_optimization/manifold_optimize.py:296-317) - with its sampling without replacement written
as the exponential race torch.multinomial runs (keys w_i / E_i, E_i ~ Exp(1), the n largest keys), and the library's counter-based random stream
(Philox4x32-10, Salmon et al. SC'11: key = seed, counter = (sample index, draw 0, tag)).  PARITY UNPINNED for the heuristic itself (botorch is not
in /root/reference and not installed: SURVEY App. B); the Philox rounds are checked against the published known-answer vectors in
tests/test_oracle_selection.py.

The library's two device samplers read the same generator and are restated here on it as well: `sphere_samples` (sphere_sample_kernel,
csrc/spd_sweep.hip) and `spd_samples` (both kernel forms of csrc/spd_sample.hip).
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
SELECT_TAG = 0x73656C65


def philox4x32_10(counter, key):
    """counter: (..., 4) uint32, key: (..., 2) uint32 -> (..., 4) uint32, ten rounds"""
    c = np.array(counter, dtype=np.uint32, copy=True)
    k = np.array(np.broadcast_to(np.asarray(key, dtype=np.uint32), c.shape[:-1] + (2,)), dtype=np.uint32, copy=True)
    mask = np.uint64(0xFFFFFFFF)
    with np.errstate(over="ignore"):
        for _ in range(10):
            p0 = M0 * c[..., 0].astype(np.uint64)
            p1 = M1 * c[..., 2].astype(np.uint64)
            n0 = (p1 >> np.uint64(32)).astype(np.uint32) ^ c[..., 1] ^ k[..., 0]
            n2 = (p0 >> np.uint64(32)).astype(np.uint32) ^ c[..., 3] ^ k[..., 1]
            c = np.stack([n0, (p1 & mask).astype(np.uint32), n2, (p0 & mask).astype(np.uint32)], axis=-1)
            k = np.stack([k[..., 0] + W0, k[..., 1] + W1], axis=-1)
    return c


def selection_uniforms(seed, total, tag=SELECT_TAG):
    """u1 in (0, 1] of draw 0 of items 0 ... total - 1 (Philox.uniform2 of gabo_philox.hpp)"""
    idx = np.arange(total, dtype=np.uint64)
    ctr = np.stack([(idx & np.uint64(0xFFFFFFFF)).astype(np.uint32), (idx >> np.uint64(32)).astype(np.uint32),
                    np.zeros(total, dtype=np.uint32), np.full(total, tag, dtype=np.uint32)], axis=-1)
    out = philox4x32_10(ctr, [np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF)])
    a = ((out[:, 0].astype(np.uint64) << np.uint64(32)) | out[:, 1].astype(np.uint64)) >> np.uint64(11)
    return (a.astype(np.float64) + 1.0) * 2.0 ** -53


def select_nonneg(y, n, seed, eta=1.0, alpha=1e-4):
    """-> (sample index of every restart (n,), keys (total,)) or (None, None) when the heuristic falls back (no positive value, fewer positive
    values than n, a NaN): exactly the cases in which the kernel raises its flag."""
    y = np.asarray(y, dtype=np.float64)
    total = y.shape[0]
    if np.isnan(y).any() or not (y.max() > 0) or int((y > 0).sum()) < n:
        return None, None
    max_idx = int(np.argmax(y))
    max_val = y[max_idx]
    thr = alpha * max_val
    while int((y >= thr).sum()) < n:
        alpha = 0.1 * alpha
        thr = alpha * max_val
    w = np.exp(eta * (y / max_val - 1.0))
    with np.errstate(divide="ignore"):
        keys = np.where(y >= thr, w / -np.log(selection_uniforms(seed, total)), -1.0)
    order = np.lexsort((np.arange(total), -keys))          # descending key, ties by the lower index
    picked = order[:n].copy()
    if max_idx not in picked:
        picked[-1] = max_idx
    return picked, keys


SPHERE_TAG = 0x73706872


def sphere_samples(seed, count, dim):
    """count points uniform on S^(dim-1) as `sphere_sample_kernel` (gabotorch_amd/csrc/spd_sweep.hip) draws them: for sample i, draw k of the Philox stream
    (seed, item i, tag "sphr") gives two uniforms (Philox.uniform2 of gabo_philox.hpp), Box-Muller two normals (coordinates 2k, 2k + 1); the row is then
    normalised - the distribution of [3P] pymanopt's Sphere.rand (randn / norm).  Agreement with the device is to rounding of log / sincospi / sqrt."""
    idx = np.arange(count, dtype=np.uint64)
    out = np.empty((count, dim), dtype=np.float64)
    key = [np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF)]
    for k in range((dim + 1) // 2):
        ctr = np.stack([(idx & np.uint64(0xFFFFFFFF)).astype(np.uint32), (idx >> np.uint64(32)).astype(np.uint32),
                        np.full(count, k, dtype=np.uint32), np.full(count, SPHERE_TAG, dtype=np.uint32)], axis=-1)
        o = philox4x32_10(ctr, key)
        a = ((o[:, 0].astype(np.uint64) << np.uint64(32)) | o[:, 1].astype(np.uint64)) >> np.uint64(11)
        b = ((o[:, 2].astype(np.uint64) << np.uint64(32)) | o[:, 3].astype(np.uint64)) >> np.uint64(11)
        u1 = (a.astype(np.float64) + 1.0) * 2.0 ** -53
        u2 = b.astype(np.float64) * 2.0 ** -53
        r = np.sqrt(-2.0 * np.log(u1))
        out[:, 2 * k] = r * np.cos(2.0 * np.pi * u2)
        if 2 * k + 1 < dim:
            out[:, 2 * k + 1] = r * np.sin(2.0 * np.pi * u2)
    return out / np.sqrt((out * out).sum(1))[:, None]


SPD_TAG = 0x6761626f
_PI_LONG = np.longdouble("3.14159265358979323846264338327950288")


def _uniform2(seed, idx, draw, tag):
    """Philox.uniform2 of gabo_philox.hpp for the items idx (uint64 array), draw number `draw`: u1 in (0, 1] from words 0 and 1, u2 in [0, 1)
    from words 2 and 3, 53 bits each, as float64 (both are exact there)"""
    idx = np.asarray(idx, dtype=np.uint64)
    ctr = np.stack([(idx & np.uint64(0xFFFFFFFF)).astype(np.uint32), (idx >> np.uint64(32)).astype(np.uint32),
                    np.full(idx.shape, draw, dtype=np.uint32), np.full(idx.shape, tag, dtype=np.uint32)], axis=-1)
    o = philox4x32_10(ctr, [np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF)])
    a = ((o[:, 0].astype(np.uint64) << np.uint64(32)) | o[:, 1].astype(np.uint64)) >> np.uint64(11)
    b = ((o[:, 2].astype(np.uint64) << np.uint64(32)) | o[:, 3].astype(np.uint64)) >> np.uint64(11)
    return (a.astype(np.float64) + 1.0) * 2.0 ** -53, b.astype(np.float64) * 2.0 ** -53


def spd_samples(seed, first, count, d, min_eig, max_eig, work=np.longdouble):
    """Samples first ... first + count - 1 of the SPD sampler (gabotorch_amd/csrc/spd_sample.hip: both of its kernel forms state the same arithmetic)
    -> (X (count, d, d) float64, lam (count, d) float64 in the order drawn, kappa (count,) float64).

    Sample i reads the Philox stream key = (seed low, seed high), counter = (index low, index high, draw, tag "gabo") with the 64-bit index first + i:
      * draws k = 0 ... ceil(d*d / 2) - 1: Box-Muller on uniform2's pair, z0 = r cos(2 pi u2), z1 = r sin(2 pi u2), r = sqrt(-2 ln u1), into the
        row-major elements 2k and 2k + 1 of the d x d Gaussian matrix (the last z1 has no element when d*d is odd);
      * its columns are orthonormalised in order: for column c two passes over p < c of dot = <q_p, q_c>, q_c -= dot q_p, then q_c /= |q_c|;
      * the eigenvalues go on with the same draw counter: draw ceil(d*d / 2) + k / 2 for k = 0, 2, 4 ... gives lam[k] = min + (max - min) u2 and
        lam[k + 1] = min + (max - min)(1 - u1) (the last one dropped when d is odd);
      * X = Q diag(lam) Q^T.
    Precision: the normals are formed in `work` and rounded to float64 - what the device holds up to the rounding of its log / sincospi / sqrt -
    and everything after them is carried in `work` (np.longdouble: 64-bit significand where the platform has one), X and lam rounded to float64 at
    the end.  work=np.float64 runs the same statements in double with numpy's libm: the oracle's check against itself.

    kappa[i] = max over the columns c of |g_c| / |r_c|, g_c the Gaussian column and r_c what both projection passes leave of it before the
    normalisation: by how much this sample amplifies a relative perturbation of its normals on the way to Q."""
    count, d = int(count), int(d)
    idx = (np.uint64(first) + np.arange(count, dtype=np.uint64)).astype(np.uint64)
    dd, two_pi = d * d, (2 * _PI_LONG if work is np.longdouble else work(2.0 * np.pi))
    g = np.zeros((count, dd + 1), dtype=np.float64)              # (one spare slot, like the register form's q[dd])
    for k in range((dd + 1) // 2):
        u1, u2 = _uniform2(seed, idx, k, SPD_TAG)
        r = np.sqrt(-2 * np.log(u1.astype(work)))
        g[:, 2 * k] = (r * np.cos(two_pi * u2.astype(work))).astype(np.float64)
        g[:, 2 * k + 1] = (r * np.sin(two_pi * u2.astype(work))).astype(np.float64)
    q = g[:, :dd].reshape(count, d, d).astype(work)
    gnorm = np.sqrt((q * q).sum(1))                              # (count, d): |g_c|
    kappa = np.ones(count, dtype=work)
    for c in range(d):
        for _ in range(2):
            for p in range(c):
                dot = (q[:, :, p] * q[:, :, c]).sum(1)
                q[:, :, c] -= dot[:, None] * q[:, :, p]
        nn = np.sqrt((q[:, :, c] * q[:, :, c]).sum(1))
        kappa = np.maximum(kappa, gnorm[:, c] / nn)
        q[:, :, c] /= nn[:, None]
    lam = np.zeros((count, d + 1), dtype=work)
    lo, width = work(min_eig), work(max_eig) - work(min_eig)
    for k in range(0, d, 2):
        u1, u2 = _uniform2(seed, idx, (dd + 1) // 2 + k // 2, SPD_TAG)
        lam[:, k] = lo + width * u2.astype(work)
        lam[:, k + 1] = lo + width * (1 - u1.astype(work))
    lam = lam[:, :d]
    x = ((q[:, :, None, :] * q[:, None, :, :]) * lam[:, None, None, :]).sum(-1)          # (q_rk q_ck first: symmetric to the last bit)
    return x.astype(np.float64), lam.astype(np.float64), kappa.astype(np.float64)
