#!/usr/bin/env python3
"""Headline benchmark: SPD affine-invariant kernel-matrix build, pairs/sec (N=4096, d=10)  [BASELINE.json metric].

A "step" = one Gram build K = SpdAffineInvariantGaussianKernel(X, X) on a synthetic set of 4096 SPD 10x10 matrices
(Mandel vectors already resident in HBM), through the C ABI of libgabo_hip.so.  Every one of the N^2 pairs is evaluated
(x1 and x2 are treated as two sets; the x1-is-x2 shortcut that evaluates only i <= j is timed separately and reported in
`symmetric_gram`, it is not `value`).

    python bench.py --gpus 1 --steps 20 --warmup 3
    python bench.py --gpus 1 --steps 20 --warmup 3 --full
    python bench.py --gpus 1 --steps 20 --warmup 3 --dump-outputs DIR
    python bench.py --gpus N ...                 (spawns its N ranks itself through torch.distributed.run, one per GPU)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

Multi-GPU: the path shards by independent Gram builds (one point set per rank, no data-path collective) -> "weak".
Prints ONE JSON line on rank 0.  `roofline` is the binding resource of the dominant kernel (fp64 issue, flop model of SURVEY 8d);
the streaming-byte model the scope contract also names is reported under `roofline_hbm_streaming_model` and marked non-physical.

A plain run does only what the headline needs: set-up, preheat and warm-up, the K timed steps, the outputs if --dump-outputs is given,
the line.  Everything else - the x1-is-x2 build, the kernel classes' forward timings, the acquisition sweeps, the other BASELINE configs,
the backward and the surrogate fit, the parity gates against the oracle, the rocprofv3 HBM-traffic passes, the CPU baseline and, with
several ranks, the collective self-check and the sharded Gram - runs with --full.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from gabotorch_amd import _lib  # noqa: E402

N_POINTS = 4096
DIM = 10
BETA = 0.2 + math.log(2.0)          # beta_min = 0.2 for d = 10 (examples/gabo_spd.py:159-160) with raw_beta = 0
BYTES_PER_PAIR = 2 * DIM * DIM * 8 + 8                 # SURVEY 8(d) streaming model: both d x d tiles + one output
FLOP_PER_PAIR = (10.0 / 3.0) * DIM ** 3 + 30.0 * DIM ** 2   # congruence + tridiagonalisation + QL
HBM_PEAK_GBS = 8000.0
FP64_PEAK_TFLOPS = 78.6
DUMP_ROWS = 1024                    # --dump-outputs: 1024 x 4096 fp64 = 32 MiB of the 128 MiB Gram


def synthetic_spd_mandel(n, d, seed):
    """eigenvalues U[0.05, 5], Q from qr(standard_normal), Mandel layout."""
    rng = np.random.default_rng(seed)
    lam = rng.uniform(0.05, 5.0, size=(n, d))
    q = np.linalg.qr(rng.standard_normal((n, d, d)))[0]
    m = np.einsum("nab,nb,ncb->nac", q, lam, q)
    m = 0.5 * (m + m.transpose(0, 2, 1))
    r, c = [], []
    for k in range(d):
        for i in range(d - k):
            r.append(i)
            c.append(i + k)
    r, c = np.array(r), np.array(c)
    return np.ascontiguousarray(m[:, r, c] * np.where(r == c, 1.0, 2.0 ** 0.5))   # (n, d_vec) row-major


class GramJob:
    """Device buffers + one C-ABI launch per step."""

    def __init__(self, x, device, symmetric):
        self.lib = _lib.load()
        self.dev = device
        self.x = torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=device).contiguous()
        n = x.shape[0]
        self.n = n
        self.out = torch.empty(n, n, dtype=torch.float64, device=device)
        self.wsb = self.lib.gabo_spd_ai_workspace_bytes(1, n, n, DIM)
        self.ws = torch.empty(self.wsb // 8, dtype=torch.float64, device=device)
        self.status = torch.zeros(2, dtype=torch.int32, device=device)
        self.flags = _lib.GABO_OUT_GAUSSIAN | (_lib.GABO_SYMMETRIC if symmetric else 0)
        self.stream = torch.cuda.current_stream(device)

    def step(self):
        rc = self.lib.gabo_spd_ai_pairwise(self.x.data_ptr(), self.x.data_ptr(), self.out.data_ptr(), None, 1, self.n, self.n, DIM,
                                           0, 0, BETA, self.flags, self.ws.data_ptr(), self.wsb, self.status.data_ptr(),
                                           self.stream.cuda_stream)
        if rc != 0:
            raise RuntimeError(f"gabo_spd_ai_pairwise failed: {rc}")


def timed(job, steps, warmup, dist):
    """W untimed steps, then exactly K steps bracketed by barrier + synchronize; returns (wall seconds, mean ms by HIP events, per-step
    ms by HIP events: one event after every step on the launch stream)."""
    for _ in range(warmup):
        job.step()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    t0 = time.perf_counter()
    ev[0].record(job.stream)
    for i in range(steps):
        job.step()
        ev[i + 1].record(job.stream)
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return wall, ev[0].elapsed_time(ev[-1]) / steps, [ev[i].elapsed_time(ev[i + 1]) for i in range(steps)]


def cpu_baseline(x):
    """The oracle's reference-faithful port (per-pair eigh loop, spd_utils_torch.py:87-120 op sequence) on a bounded
    sample of the same workload: the first `rows` rows of the Gram matrix against all columns.  Timed twice: torch pinned to ONE
    thread (`value`, `cores` = 1: the per-pair loop is scalar, so this is what the reference's structure can use) and with every
    host core offered to torch (`all_threads`: the 10 x 10 eigh calls do not parallelise, extra threads only add overhead)."""
    from oracle import spd as ospd
    rows = 320
    prev_threads = torch.get_num_threads()
    torch.set_num_threads(1)
    t0 = time.perf_counter()
    k = ospd.spd_ai_gaussian_kernel(x[:rows], x, BETA, faithful=True)
    dt = time.perf_counter() - t0
    ncpu = os.cpu_count() or 1
    rows_all = 96
    torch.set_num_threads(ncpu)
    t2 = time.perf_counter()
    ka = ospd.spd_ai_gaussian_kernel(x[:rows_all], x, BETA, faithful=True)
    dta = time.perf_counter() - t2
    torch.set_num_threads(prev_threads)
    assert np.allclose(ka, k[:rows_all], rtol=1e-9, atol=1e-14)
    # context line: the same arithmetic vectorised on the CPU (batched LAPACK eigvalsh), not what the reference does
    vrows = 64
    t1 = time.perf_counter()
    kv = ospd.spd_ai_gaussian_kernel(x[:vrows], x, BETA, faithful=False)
    dtv = time.perf_counter() - t1
    assert np.allclose(kv, k[:vrows], rtol=1e-9, atol=1e-14)
    ref_proper = None
    try:
        rp = json.load(open(os.path.join(ROOT, "profiles", "r04_reference_cpu.json")))
        ref_proper = {"pairs_per_s": rp["spd_config3"]["pairs_per_s"], "cores": rp["host"]["cores"], "kind": "reference",
                      "where": "the reference ITSELF (its Mandel loop + affine_invariant_distance_torch + exp) on the config-3 input in the build container, "
                               "8 vCPU / 8 torch threads, tools/time_reference_cpu.py -> profiles/r04_reference_cpu.json; /root/reference does not travel to the "
                               "GPU box, so this figure is not re-timed here"}
    except Exception:       # noqa: BLE001
        pass
    return {"value": rows * x.shape[0] / dt, "unit": "pairs/s", "cores": 1, "kind": "port",
            "reference_proper_pairs_per_s": None if ref_proper is None else ref_proper["pairs_per_s"], "reference_proper": ref_proper,
            "all_threads": {"value": rows_all * x.shape[0] / dta, "unit": "pairs/s", "cores": ncpu, "torch_threads": ncpu,
                            "sample": f"first {rows_all} Gram rows ({rows_all * x.shape[0]} pairs, {dta:.1f} s)"},
            "vectorised_numpy_pairs_per_s": vrows * x.shape[0] / dtv,
            "sample": f"first {rows} of {x.shape[0]} Gram rows x all {x.shape[0]} columns ({rows * x.shape[0]} pairs, {dt:.1f} s): "
                      "oracle.spd.affine_invariant_distance_faithful = the reference's op sequence (Mandel->matrix by its per-vector Python loop, "
                      "Cholesky, inverse, two bmm, one torch.linalg.eigh per pair in a Python loop, exp), torch CPU fp64, one thread (the loop is "
                      "scalar); the reference itself on this input, build container, 8 threads: 3.74e4 pairs/s (profiles/r04_reference_cpu.json)",
            "host_cpus": ncpu}, k


def measure_hbm_traffic(timeout_s=150):
    """HBM bytes per launch of the headline kernel from the PMC counters, measured in THIS run: two rocprofv3 passes (FETCH_SIZE and WRITE_SIZE do
    not fit one pass: MI355X_MICROARCH.md, counter table) over three launches of the same N = 4096, d = 10 Gram build (tools/prof_spd.py), only
    --kernel-trace next to --pmc.  Units and gfx950 corrections as the guide prescribes: the counters are in KB; FETCH_SIZE under-reports coalesced
    streaming reads on gfx950 by the factor calibrated on a kernel of known byte count (profiles/pmc_summary.json `fetch_calibration`: 2.013).
    Returns (bytes_per_launch or None, description)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3")
    if exe is None:
        return None, "rocprofv3 not on PATH"
    if any(k.startswith(("ROCP_", "ROCPROF", "ROCPROFILER")) for k in os.environ):
        return None, "this process is itself running under a profiler"
    factor = 2.013135990798753
    try:
        factor = float(json.load(open(os.path.join(ROOT, "profiles", "pmc_summary.json")))["fetch_calibration"]["factor"])
    except Exception:       # noqa: BLE001
        pass
    env = {k: v for k, v in os.environ.items() if not k.startswith(("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_"))}
    env["TMPDIR"] = "/tmp"
    got = {}
    work = tempfile.mkdtemp(prefix="gabo_pmc_", dir="/tmp")
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(work, counter)
            cmd = [exe, "--pmc", counter, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "out", "--",
                   sys.executable, os.path.join(ROOT, "tools", "prof_spd.py"), str(N_POINTS), str(DIM), "x", "3"]
            try:
                subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=timeout_s)
            except subprocess.TimeoutExpired:
                return None, f"rocprofv3 --pmc {counter} pass exceeded {timeout_s} s"
            files = glob.glob(d + "/**/out_counter_collection.csv", recursive=True)
            if not files:
                return None, f"rocprofv3 --pmc {counter} pass wrote no counter file"
            vals = [float(r["Counter_Value"]) for r in csv.DictReader(open(files[0]))
                    if "spd_ai_pairwise_kernel" in r["Kernel_Name"] and r["Counter_Name"] == counter]
            if not vals:
                return None, f"no spd_ai_pairwise_kernel dispatch in the {counter} pass"
            got[counter] = sum(vals) / len(vals)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    total = got["FETCH_SIZE"] * 1024.0 * factor + got["WRITE_SIZE"] * 1024.0
    return total, (f"measured in this run: rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE in separate passes (with --kernel-trace only) over 3 launches of "
                   f"the same Gram build; KB -> B; FETCH_SIZE x {factor:.3f} (gfx950 under-report of coalesced reads, calibrated on a kernel of known "
                   f"byte count: profiles/pmc_summary.json); raw KB per launch: FETCH_SIZE {got['FETCH_SIZE']:.0f}, WRITE_SIZE {got['WRITE_SIZE']:.0f}")


def config5_pieces(device):
    """BASELINE.json config 5 at its stated size: N = 4096 points of S^20_++ projected to S^2_++ (Y = W^T X W, nested_spd_utils.py:13-48)
    followed by the nested affine-invariant Gram and the log-Euclidean Gram of the latent points; parity of a block against the oracle."""
    from gabotorch_amd import _lib, ops as _ops
    from oracle import spd as ospd
    n, D, d = N_POINTS, 20, 2
    xm = synthetic_spd_mandel(n, D, 1234)
    rng = np.random.default_rng(4321)
    W = np.ascontiguousarray(np.linalg.qr(rng.standard_normal((D, D)))[0][:, :d])
    x, w = torch.tensor(xm, device=device), torch.tensor(W, device=device)
    beta5 = 0.6 + math.log(2.0)                     # beta_min of S^2_++ (examples/gabo_spd.py:151-152)

    def ev_ms(fn, iters=20):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    def graph_ms(fn, reps=10, replays=5):
        """device time per call without the host's launch overhead (which bounds `ev_ms` for the 5-10 us kernels): `reps` calls captured
        into one hipGraph, replayed `replays` times between two events"""
        prev = _ops.set_error_checking(False)    # (the status read-back is a host synchronisation: not capturable)
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                fn()
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(reps):
                    fn()
            g.replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(replays):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / (reps * replays)
        finally:
            _ops.set_error_checking(prev)
    ms_p = ev_ms(lambda: _ops.spd_project(x, w))
    y = _ops.spd_project(x, w)
    ms_ai = ev_ms(lambda: _ops.spd_ai_pairwise(y, y, beta=beta5))
    ms_lg = ev_ms(lambda: _ops.spd_logm_mandel(y))
    lg = _ops.spd_logm_mandel(y)
    ms_le = ev_ms(lambda: _ops.frobenius_pairwise(lg, lg, beta=1.0))
    dev_ms = {"projection": graph_ms(lambda: _ops.spd_project(x, w)), "nested_ai_gram": graph_ms(lambda: _ops.spd_ai_pairwise(y, y, beta=beta5)),
              "logm": graph_ms(lambda: _ops.spd_logm_mandel(y)), "log_euclidean_gram": graph_ms(lambda: _ops.frobenius_pairwise(lg, lg, beta=1.0))}
    # the two Gram builds of the nested kernels from the ORIGINAL points in two launches each (gabo_nested_spd_gram: projection + factorisation /
    # logm fused into one launch, then the Gram launch)
    dev_ms["nested_ai_gram_from_original_points"] = graph_ms(lambda: _ops.nested_spd_gram(x, x, w, beta5, _lib.GABO_METRIC_AFFINE_INVARIANT))
    dev_ms["nested_log_euclidean_gram_from_original_points"] = graph_ms(lambda: _ops.nested_spd_gram(x, x, w, 1.0, _lib.GABO_METRIC_LOG_EUCLIDEAN))
    e_fused = float(max((_ops.nested_spd_gram(x[:96], x[:96], w, beta5, _lib.GABO_METRIC_AFFINE_INVARIANT) - _ops.spd_ai_pairwise(y[:96], y[:96], beta=beta5)).abs().max(),
                        (_ops.nested_spd_gram(x[:96], x[:96], w, 1.0, _lib.GABO_METRIC_LOG_EUCLIDEAN) - _ops.frobenius_pairwise(lg[:96], lg[:96], beta=1.0)).abs().max()))
    if not e_fused < 1e-12:
        raise RuntimeError(f"config 5 fused Gram differs from the separate-launch chain: {e_fused}")
    # parity: projection, then both Gram blocks against the oracle
    xs = ospd.vector_to_symmetric_matrix_mandel(xm[:96])
    yo = ospd.symmetric_matrix_to_vector_mandel(ospd.projection_from_spd_to_nested_spd(xs, W))
    e_p = float(np.max(np.abs(y[:96].cpu().numpy() - yo)))
    kai = _ops.spd_ai_pairwise(y[:96], y[:96], beta=beta5).cpu().numpy()
    e_ai = float(np.max(np.abs(kai - ospd.spd_ai_gaussian_kernel(yo, yo, beta5))))
    kle = _ops.frobenius_pairwise(lg[:96], lg[:96], beta=1.0).cpu().numpy()
    e_le = float(np.max(np.abs(kle - ospd.log_euclidean_gaussian_kernel(yo, yo, 1.0))))
    if not (e_p < 1e-10 and e_ai < 1e-9 and e_le < 1e-9):
        raise RuntimeError(f"config 5 parity gate failed: {e_p} {e_ai} {e_le}")
    # the latent loop of an HD-GaBO iteration at D = 20: one reconstruction evaluation (value + gradients, 13 data points: the fused
    # launch of nested_spd_optimization.py:23-92) and the original-space eigenvalue constraints of 512 latent points (one launch:
    # nested_spd_constraints_utils.py:14-73), each checked against the oracle
    nd = 13
    xd = ospd.vector_to_symmetric_matrix_mandel(xm[:nd])
    Rm = np.linalg.qr(rng.standard_normal((D, D)))[0]
    Wl, Vl = np.ascontiguousarray(Rm[:, :d]), np.ascontiguousarray(Rm[:, d:])
    qc = np.linalg.qr(rng.standard_normal((D - d, D - d)))[0]
    Cl = (qc * rng.uniform(0.5, 2.0, D - d)) @ qc.T
    Kl = rng.standard_normal((d, D - d))
    Kl *= 0.4 / np.linalg.norm(Kl)
    yd = np.einsum("ab,nac,cd->nbd", Wl, xd, Wl)
    T64 = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=device)   # noqa: E731
    rec = _ops.NestedSpdReconstruction(T64(xd), T64(yd), T64(Wl), _lib.GABO_RECON_LOG_EUCLIDEAN)
    vt, ct, kt = T64(Vl), T64(Cl), T64(Kl)
    cost_t, gv_t, gc_t, gk_t = torch.empty(1, dtype=torch.float64, device=device), torch.empty_like(vt), torch.empty_like(ct), torch.empty_like(kt)
    ws_rec = rec._staging(1)["ws"]
    ms_rec = graph_ms(lambda: rec.launch(vt, ct, kt, cost_t, gv_t, gc_t, gk_t, 1, ws_rec), reps=5)
    e_rec = abs(float(cost_t[0]) - ospd.reconstruction_cost(xd, yd, Wl, Vl, Cl, Kl, metric="le")) / abs(float(cost_t[0]))
    lw, lx0, lp = _ops.nested_spd_lift_prepare(T64(Wl), vt, ct, kt)
    ylat = _ops.mandel_to_matrix(y[:512])
    ms_nc = graph_ms(lambda: _ops.nested_spd_extreme_eigenvalues(ylat, lw, lp, lx0, want_grad=True), reps=5)
    lam_nc = _ops.nested_spd_extreme_eigenvalues(ylat[:64], lw, lp, lx0).cpu().numpy()
    lam_o = np.linalg.eigvalsh(ospd.projection_from_nested_spd_to_spd(ylat[:64].cpu().numpy(), Wl, Vl, Cl, Kl))
    e_nc = float(max(np.abs(lam_nc[:, 0] - lam_o[:, -1]).max(), np.abs(lam_nc[:, 1] - lam_o[:, 0]).max()))
    if not (e_rec < 1e-10 and e_nc < 1e-11):
        raise RuntimeError(f"config 5 latent-loop parity gate failed: {e_rec} {e_nc}")
    # the whole optimisation of the reconstruction parameters from this start (augmented Lagrangian + conjugate gradients as a native host
    # loop around the launch above: gabo_nested_spd_reconstruction_solve), the example's settings (6 outer iterations, 100 inner)
    opts = _lib.ReconSolveOptions(bound=20, rho_init=1, thetarho=0.3, tau=0.8, starting_tolgradnorm=1e-3, ending_tolgradnorm=1e-6, gammas_fact=1.0,
                                  minstepsize=1e-10, maxtime=1000, maxiter=6, cg_minstepsize=1e-10, cg_maxtime=1000, cg_orth_value=float("inf"),
                                  cg_maxiter=100)
    unit0 = Kl.reshape(-1) / np.linalg.norm(Kl)
    raw0 = float(np.log(0.4 / 0.6))                                     # sigmoid(raw) = 0.4 = ||K||
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        v_o, c_o, u_o, r_o, slog = rec.solve_host(Vl, Cl, unit0, raw0, opts)
        wall = time.perf_counter() - t0
        best = wall if best is None else min(best, wall)
    k_o = u_o.reshape(d, D - d) / (1.0 + np.exp(-r_o[0]))
    e_sol = abs(slog["final_cost"] - ospd.reconstruction_cost(xd, yd, Wl, v_o, c_o, k_o, metric="le")) / abs(slog["final_cost"])
    if not (e_sol < 1e-9 and slog["final_cost"] <= float(cost_t[0]) and np.linalg.eigvalsh(c_o).min() > 0):
        raise RuntimeError(f"config 5 reconstruction-loop gate failed: {e_sol} {slog}")
    solve = {"wall_ms": best * 1e3, "launches": slog["launches"], "evaluations": slog["evaluations"], "inner_iterations": slog["inner_iterations"],
             "us_per_launch": best * 1e6 / max(slog["launches"], 1), "start_cost": float(cost_t[0]), "final_cost": slog["final_cost"],
             "constraint_violation": slog["violation"], "final_cost_vs_oracle_rel": e_sol}
    pairs = n * n
    hbm = lambda nbytes, ms: {"bound": "hbm", "achieved": nbytes / (ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",   # noqa: E731
                              "frac": nbytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS}
    return {"workload": "hd_gabo_spd pieces, N=4096: projection S^20_++ -> S^2_++ (W from qr(randn), seed 4321), nested affine-invariant "
                        "Gram (beta=0.6+ln2), logm of the latent points, log-Euclidean Gram (lengthscale 1)",
            "projection_ms": ms_p, "projection_matrices_per_s": n / (ms_p * 1e-3),
            "projection_roofline": dict(hbm(n * (D * (D + 1) // 2 + 3) * 8, ms_p),
                                        model="one read of the 210-entry Mandel vector + one write of the 3-entry result per matrix"),
            "nested_ai_gram_ms": ms_ai, "nested_ai_gram_pairs_per_s": pairs / (ms_ai * 1e-3),
            "nested_ai_gram_roofline": dict(hbm(pairs * 8.0, ms_ai), model="8 algorithmic B/pair: one fp64 output (2 x 2 operands are L2-resident)"),
            "logm_ms": ms_lg,
            "log_euclidean_gram_ms": ms_le, "log_euclidean_gram_pairs_per_s": pairs / (ms_le * 1e-3),
            "log_euclidean_gram_roofline": dict(hbm(pairs * 8.0, ms_le), model="8 algorithmic B/pair: one fp64 output"),
            "device_ms_in_a_hip_graph": dict(dev_ms, note="the *_ms figures above are HIP events around 20 calls issued from the host: for the "
                                             "5-10 us kernels that is the host's launch rate; these are the same calls captured in one hipGraph"),
            "latent_loop": {"workload": "D = 20 -> 2: one reconstruction evaluation (value + gradients w.r.t. V, C, K; 13 data points, log-Euclidean "
                                        "cost; gabo_nested_spd_reconstruction) and lambda_max / lambda_min of 512 lifted latent points with their "
                                        "gradients (gabo_nested_spd_extreme_eigenvalues); device ms per launch inside a hipGraph",
                            "reconstruction_evaluation_ms": ms_rec, "nested_eigenvalue_constraints_512_points_ms": ms_nc,
                            "reconstruction_optimisation": solve,
                            "bound": "latency: two dependent eigen-solves of order 18 and 20 per block (wave_eigh: one wave, ~2.1e5 shader cycles); "
                                     "one Householder reduction + multisection per lifted point (~6e4 cycles)",
                            "parity": {"reconstruction_cost_rel": e_rec, "extreme_eigenvalues_max_abs": e_nc}},
            "parity": {"projection_max_abs": e_p, "nested_ai_gram_max_abs": e_ai, "log_euclidean_gram_max_abs": e_le, "block": "96 x 96"}}


def hd_sphere_pieces(device):
    """The nested-sphere chain of HD-GaBO on the sphere (examples/hd_bo_sphere/benchmark_examples/hd_gabo_sphere.py) at D = 51 -> 3 (48 levels):
    all levels of the projection for N = 4096 points in one launch, and one reconstruction evaluation (lift + geodesic distance + gradient
    w.r.t. the 48 distances) of 64 data points; each checked against the oracle."""
    from gabotorch_amd import _lib, ops as _ops
    from oracle import sphere as osph
    lib = _lib.load()
    D, lat, n = 51, 3, N_POINTS
    L = D - lat
    rng = np.random.default_rng(5151)
    axes_np = []
    for k in range(L):
        a = rng.standard_normal(D - k)
        axes_np.append(a / np.linalg.norm(a))
    r_np = rng.uniform(0.8, 2.2, L)
    x = rng.standard_normal((n, D))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    xt = torch.tensor(x, device=device)
    axes = [torch.tensor(a, device=device) for a in axes_np]
    frames, dists = _ops._nested_sphere_frames(axes, list(r_np), D, device)
    z = torch.empty(n, lat, dtype=torch.float64, device=device)
    stream = _ops._stream_ptr(device)

    def ev_ms(fn, iters=20):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters
    ms_proj = ev_ms(lambda: lib.gabo_nested_sphere_project(xt.data_ptr(), frames.data_ptr(), dists.data_ptr(), z.data_ptr(), None, n, D, L, stream))
    e_proj = float(np.max(np.abs(z[:64].cpu().numpy() - osph.projection_from_sphere_to_subsphere(x[:64], axes_np, r_np)[-1])))
    nd = 64
    rec = _ops.NestedSphereReconstruction(xt[:nd], z[:nd], axes)
    rd = torch.tensor(r_np, device=device)
    out = torch.empty(1 + L, dtype=torch.float64, device=device)
    ws = torch.empty(max(int(lib.gabo_nested_sphere_reconstruction_workspace_bytes(1, nd, D, L)), 16), dtype=torch.uint8, device=device)
    ms_rec = ev_ms(lambda: lib.gabo_nested_sphere_reconstruction(rec.x.data_ptr(), rec.z.data_ptr(), rec.frames.data_ptr(), rd.data_ptr(), out.data_ptr(),
                                                                 out[1:].data_ptr(), 1, nd, D, L, ws.data_ptr(), ws.numel(), stream))
    want = osph.nested_sphere_reconstruction_cost(x[:nd], z[:nd].cpu().numpy(), axes_np, r_np)
    e_rec = abs(float(out[0]) - want) / abs(want)
    if not (e_proj < 1e-9 and e_rec < 1e-9):
        raise RuntimeError(f"nested-sphere parity gate failed: {e_proj} {e_rec}")
    # algorithmic traffic of the projection: one read of the point, one write of the latent point; the frames (10 KB) stay in L2
    nbytes = n * (D + lat) * 8
    return {"workload": "hd_gabo_sphere pieces, D = 51 -> 3 (48 nested levels): projection of N=4096 points through all levels (one wave per point); "
                        "one reconstruction evaluation with its gradient w.r.t. the 48 distances, 64 data points",
            "projection_ms": ms_proj, "projection_points_per_s": n / (ms_proj * 1e-3),
            "projection_roofline": {"bound": "latency: 48 dependent levels per wave (one inner product, one acos / sin, one norm each)",
                                    "achieved": nbytes / (ms_proj * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                    "frac": nbytes / (ms_proj * 1e-3) / 1e9 / HBM_PEAK_GBS},
            "reconstruction_evaluation_ms": ms_rec,
            "parity": {"projection_max_abs": e_proj, "reconstruction_cost_rel": e_rec}}


def plugin_surface_timings(device, x, kernel_ms, steps):
    """What a GaBOtorch user calls (`kernel.forward(X, X)`), timed next to the C-ABI launch the headline times: the kernel classes'
    `forward` on the headline point set under torch.no_grad() and with X.requires_grad_(), HIP events on torch's current stream, `steps` calls each
    after 3 untimed ones.  kernels_spd.py:72-100 / kernels_sphere.py:71-94 of the reference."""
    from gabotorch_amd.kernel_utils.kernels_spd import SpdAffineInvariantGaussianKernel
    from gabotorch_amd.kernel_utils.kernels_sphere import SphereGaussianKernel

    def ev_ms(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
        ev[0].record()
        for i in range(steps):
            fn()
            ev[i + 1].record()
        torch.cuda.synchronize()
        per = [ev[i].elapsed_time(ev[i + 1]) for i in range(steps)]
        return float(np.mean(per)), float(np.median(per))

    out = {}
    kern = SpdAffineInvariantGaussianKernel(beta_min=0.2)            # beta = softplus(0) + 0.2 = BETA (parameter on the host, as the examples keep it)
    X = torch.tensor(np.ascontiguousarray(x), device=device)
    X2 = X.clone()
    with torch.no_grad():
        same = ev_ms(lambda: kern.forward(X, X))
        full = ev_ms(lambda: kern.forward(X, X2))
        want = ops_pairwise_reference(X, X2, float(kern.beta.double()))
        err = float((kern.forward(X, X2) - want).abs().max())
        err_same = float((kern.forward(X, X) - want).abs().max())
    Xg = X.clone().requires_grad_()
    grad = ev_ms(lambda: kern.forward(Xg, X2))
    nbytes = float(X.shape[0]) ** 2 * 8
    out["spd"] = {
        "class": "SpdAffineInvariantGaussianKernel(beta_min=0.2)", "n_points": int(X.shape[0]), "dim": DIM,
        "forward_ms_no_grad_x_is_x": same[0], "forward_ms_no_grad_x_is_x_median": same[1],
        "forward_ms_no_grad": full[0], "forward_ms_no_grad_median": full[1],
        "forward_ms_grad_enabled": grad[0], "forward_ms_grad_enabled_median": grad[1],
        "c_abi_kernel_ms": kernel_ms,
        "overhead_no_grad_vs_c_abi": full[0] / kernel_ms - 1.0,
        "overhead_grad_enabled_vs_c_abi": grad[0] / kernel_ms - 1.0,
        "max_abs_diff_vs_c_abi_output": err, "max_abs_diff_x_is_x_vs_c_abi_output": err_same,
        "note": "forward(X, X) with the SAME tensor takes the x1-is-x2 build (i <= j evaluated, mirrored: half the pairs - what a GP's train-train Gram "
                "is); forward(X, X.clone()) evaluates all N^2 pairs like `value`: the class path adds the output allocation and a few us of Python to "
                "the launch.  With a gradient requested the launch also writes the distance matrix (a second N^2 x 8 B = "
                f"{nbytes / 1e6:.0f} MB store, kept for the beta-gradient) and uses the strict QL deflation threshold (both outputs leave the kernel)"}
    rng = np.random.default_rng(1234)
    sx = rng.standard_normal((N_POINTS, 10))
    sx /= np.linalg.norm(sx, axis=1, keepdims=True)
    S = torch.tensor(sx, device=device)
    S2 = S.clone()
    sk = SphereGaussianKernel(beta_min=0.6)
    from gabotorch_amd import ops as _o
    with torch.no_grad():
        for _ in range(200):                 # (write-bound: the clocks settle over a few hundred launches, see sphere_gram below)
            sk.forward(S, S2)
        s_full = ev_ms(lambda: sk.forward(S, S2))
        s_abi = ev_ms(lambda: _o.sphere_pairwise(S, S2, beta=0.6 + float(np.log(2.0))))
    Sg = S.clone().requires_grad_()
    s_grad = ev_ms(lambda: sk.forward(Sg, S2))
    out["sphere"] = {"class": "SphereGaussianKernel(beta_min=0.6)", "n_points": N_POINTS, "dim": 10,
                     "forward_ms_no_grad": s_full[0], "forward_ms_no_grad_median": s_full[1],
                     "forward_ms_grad_enabled": s_grad[0], "forward_ms_grad_enabled_median": s_grad[1],
                     "ops_sphere_pairwise_ms_same_conditions": s_abi[0],
                     "overhead_no_grad_vs_ops_call": s_full[0] / s_abi[0] - 1.0,
                     "note": "same stream and clock state for the class call and the ops call (the sustained figure of `sphere_gram` is taken on a private "
                             "stream after 600 launches); with a gradient requested the autograd wrapper saves the inner products for the backward"}
    return out


def ops_pairwise_reference(X, X2, beta):
    """the C-ABI launch `value` times, with the kernel object's own beta (an fp32 parameter: softplus(0) + 0.2 to 1e-8 of BETA)"""
    from gabotorch_amd import ops as _o
    return _o.spd_ai_pairwise(X, X2, beta=beta)


def _collective_selfcheck(dist, device, world, rank):
    """The collectives of the data path executed once each on the initialised backend with the shapes the path uses, results
    checked, durations reported: the row-block slab of the sharded Gram (all_gather_into_tensor), the packed (value, candidate) rows of the
    restarts and of the raw samples (all_gather into a list), the max-over-ranks reduction of the timings, the barrier."""
    out = {}

    def timed_ms(fn, reps=3):
        fn()
        torch.cuda.synchronize()
        dist.barrier()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3

    per = (N_POINTS + world - 1) // world
    slab = torch.full((per, N_POINTS), float(rank), dtype=torch.float64, device=device)
    full = torch.empty(world * per, N_POINTS, dtype=torch.float64, device=device)
    try:
        out["all_gather_into_tensor_gram_slab_ms"] = timed_ms(lambda: dist.all_gather_into_tensor(full, slab))
    except (RuntimeError, NotImplementedError, AttributeError):      # gloo (the one-device test hook): the list form, as distributed.sharded_gram does
        slabs = [torch.empty_like(slab) for _ in range(world)]
        out["all_gather_into_tensor_gram_slab_ms"] = timed_ms(lambda: dist.all_gather(slabs, slab))
        out["gram_slab_collective"] = "all_gather (list form)"
        full = torch.cat(slabs)
    want = torch.arange(world, dtype=torch.float64, device=device).repeat_interleave(per)
    ok = bool(torch.equal(full[:, 0], want) and torch.equal(full[:, -1], want))
    packed = torch.full((512 // world + 1, 16), float(rank), dtype=torch.float64, device=device)
    parts = [torch.empty_like(packed) for _ in range(world)]
    out["all_gather_restart_rows_ms"] = timed_ms(lambda: dist.all_gather(parts, packed))
    ok = ok and all(bool((parts[r] == float(r)).all()) for r in range(world))
    t = torch.tensor([float(rank)], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    ok = ok and float(t.item()) == float(world - 1)
    dist.barrier()
    out["bytes_gram_slab_per_rank"] = per * N_POINTS * 8
    out["ok"] = ok
    if not ok:
        raise RuntimeError(f"collective self-check failed on backend {dist.get_backend()}")
    return out


def _self_launch(args):
    """`python bench.py --gpus N` without a torch.distributed.run environment: start the N ranks (one process per GPU, RCCL over
    xGMI) and relay their output - rank 0 prints the JSON line."""
    import socket
    import subprocess
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    raise SystemExit(subprocess.run(cmd, env=env).returncode)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--preheat", type=int, default=60, help="untimed launches BEFORE the W warm-up steps: a cold MI355X needs ~20 launches "
                    "(~60 ms) of fp64 load to reach its sustained clock (rocprofv3: 3.30 ms for the first dispatch, 2.67 ms from the "
                    "20th on, profiles/pmc_summary.json); reported in the line as `untimed_preheat_steps`")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--traffic", choices=["auto", "measure", "file"], default="auto", help="roofline.traffic: measured in this run with two rocprofv3 "
                    "--pmc passes (auto: with --full, when rocprofv3 is on PATH, one rank, not already under a profiler; ~30 s) or read from "
                    "profiles/pmc_summary.json")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--sweep-lite", action="store_true", help="only the single-launch-solve variants of the config-4 sweep (tests: the eight-rank run on one device)")
    ap.add_argument("--no-plugin-surface", action="store_true", help="skip the kernel classes' forward timings (profiling runs)")
    ap.add_argument("--no-symmetric", action="store_true", help="skip the separately reported x1-is-x2 run (profiling: keeps "
                    "the rocprof average of the pairwise kernel equal to the `value` launches)")
    ap.add_argument("--full", action="store_true", help="also measure and check everything beside the headline (see the module docstring); "
                    "the --no-* options and --sweep-lite select within it")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write what the last step computed on rank 0 to DIR/gram_rows.npy: "
                    f"{DUMP_ROWS} rows of the {N_POINTS} x {N_POINTS} Gram (a fixed seeded sample, ascending), float64")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if world > 1 or "RANK" in os.environ:      # under torchrun the RCCL path is exercised even with one rank
        import torch.distributed as dist_mod
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if os.environ.get("GABO_BENCH_ONE_DEVICE"):
            # test hook: exercise the multi-rank code paths on a ONE-GPU box (all ranks on cuda:0, gloo instead of RCCL, which
            # refuses two ranks on one device); never set by the driver
            local_rank = 0
            torch.cuda.set_device(0)
            dist_mod.init_process_group("gloo")
        else:
            torch.cuda.set_device(local_rank)
            dist_mod.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        dist = dist_mod
    elif args.gpus != 1:
        _self_launch(args)
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)
    backend = "none" if dist is None else str(dist.get_backend())
    collectives = None if dist is None or not args.full else _collective_selfcheck(dist, device, world, rank)

    x = synthetic_spd_mandel(N_POINTS, DIM, 1234 + rank)      # one independent point set per rank
    job = GramJob(x, device, symmetric=False)
    for _ in range(max(args.preheat, 0)):
        job.step()
    torch.cuda.synchronize()
    wall, ev_ms, step_ms = timed(job, args.steps, args.warmup, dist)
    st = job.status.tolist()
    if st[0] != 0:
        raise RuntimeError(f"device status {st}")
    if args.dump_outputs and rank == 0:
        os.makedirs(args.dump_outputs, exist_ok=True)
        rows = np.sort(np.random.default_rng(0).choice(N_POINTS, DUMP_ROWS, replace=False))
        np.save(os.path.join(args.dump_outputs, "gram_rows.npy"), job.out[torch.from_numpy(rows).to(device)].cpu().numpy())
    sym, sym_ms = None, None
    if args.full and not args.no_symmetric:
        sym = GramJob(x, device, symmetric=True)
        _, sym_ms, _ = timed(sym, args.steps, args.warmup, None)

    plugin = None
    if args.full and rank == 0 and world == 1 and not args.no_plugin_surface:
        plugin = plugin_surface_timings(device, x, ev_ms, args.steps)

    sharded = None
    if args.full and world > 1:
        # strong scaling of ONE N=4096 Gram: row blocks over the ranks, left sharded or assembled with one all_gather
        from gabotorch_amd import ops as _ops
        from gabotorch_amd.distributed import sharded_gram
        xs = torch.tensor(np.ascontiguousarray(synthetic_spd_mandel(N_POINTS, DIM, 1234)), device=device)
        fwd = lambda a, b: _ops.spd_ai_pairwise(a, b, beta=BETA)       # noqa: E731
        res = {}
        for gather in (False, True):
            for _ in range(3):
                sharded_gram(fwd, xs, xs, gather=gather)
            torch.cuda.synchronize()
            dist.barrier()
            t0 = time.perf_counter()
            for _ in range(10):
                sharded_gram(fwd, xs, xs, gather=gather)
            torch.cuda.synchronize()
            dist.barrier()
            tt = torch.tensor([(time.perf_counter() - t0) / 10], dtype=torch.float64, device=device)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            res["all_gathered" if gather else "left_sharded"] = {"ms": float(tt.item()) * 1e3, "pairs_per_s": N_POINTS * N_POINTS / float(tt.item())}
        full = fwd(xs, xs)
        err_sh = float((sharded_gram(fwd, xs, xs, gather=True) - full).abs().max().item())
        sharded = {"workload": "one N=4096 d=10 Gram, row blocks of x1 over the ranks (replicated inputs)", **res,
                   "parity_max_abs_vs_unsharded": err_sh}

    sweep = None
    if args.full and not args.no_sweep:
        # config 4 (gabo_spd S^5_++, 512 restarts): lock-step trust regions, restarts sharded r % world over the ranks,
        # one all_gather + argmax (RCCL).  Reported beside the headline metric, never mixed into `value`.
        from tools.sweep_bench import run_sweep
        run_sweep(device, num_restarts=512, batched_rand=True, builtin_constraint=True)   # warm-up (allocator, code objects)
        if dist is not None:
            dist.barrier()
        sw_s0, sw_best, sw_val, sw_log = run_sweep(device, num_restarts=512, batched_rand=True, builtin_constraint=True)
        lite = args.sweep_lite
        sw_l = None if lite else run_sweep(device, num_restarts=512, hip_graphs=True, batched_rand=True)[0]        # the same constraint as an opaque lambda
        tt = torch.tensor([sw_s0], dtype=torch.float64, device=device)
        if dist is not None:
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        if lite:
            sw_c = sw_val_c = sw_d = sw_val_d = None
        else:
            sw_c, _, sw_val_c, _ = run_sweep(device, num_restarts=512, hip_graphs=True, batched_rand=True, capture_constraints=True)
            sw_d = min(run_sweep(device, num_restarts=512, hip_graphs=True, device_rand=True, capture_constraints=True)[0] for _ in range(3))
            sw_val_d = run_sweep(device, num_restarts=512, hip_graphs=True, device_rand=True, capture_constraints=True)[2]
        # the constraint given as functools.partial(max_eigenvalue_constraint_torch, ...) like the reference example does
        # (examples/gabo_spd.py:136-138): evaluated on the device, the whole solve is one launch (gabo_spd_tr_solve)
        sw_s = min(run_sweep(device, num_restarts=512, batched_rand=True, builtin_constraint=True)[0] for _ in range(3))
        sw_sd = min(run_sweep(device, num_restarts=512, device_rand=True, builtin_constraint=True)[0] for _ in range(3))
        # (the same sweep with the native host driver switched off: joint_optimize_manifold's Python path, launch for launch the same work)
        sw_sd_py = min(run_sweep(device, num_restarts=512, device_rand=True, builtin_constraint=True, native_sweep=False)[0] for _ in range(3))
        sw_val_sd_py = run_sweep(device, num_restarts=512, device_rand=True, builtin_constraint=True, native_sweep=False)[2]
        sw_val_s = run_sweep(device, num_restarts=512, batched_rand=True, builtin_constraint=True)[2]
        ts = torch.tensor([sw_s, sw_sd, sw_sd_py], dtype=torch.float64, device=device)
        if dist is not None:
            dist.all_reduce(ts, op=dist.ReduceOp.MAX)
        sw_s, sw_sd, sw_sd_py = float(ts[0]), float(ts[1]), float(ts[2])
        # (device sampler: every rank holds the same seed and draws its index range of the SAME stream, so this value does not
        # depend on the number of ranks - tests/test_gpu_multirank_bench.py compares it with the single-rank run)
        sw_val_sd = run_sweep(device, num_restarts=512, device_rand=True, builtin_constraint=True)[2]
        weak = None
        if world > 1:
            # weak scaling of the same sweep: 512 restarts PER GPU (the 512-restart sweep itself is latency-bound on one GPU)
            kw = dict(num_restarts=512 * world, raw_samples=2048 * world, device_rand=True, builtin_constraint=True)
            run_sweep(device, **kw)
            dist.barrier()
            ww = torch.tensor([run_sweep(device, **kw)[0]], dtype=torch.float64, device=device)
            dist.all_reduce(ww, op=dist.ReduceOp.MAX)
            weak = {"restarts": 512 * world, "seconds": float(ww.item()), "restarts_per_s": 512 * world / float(ww.item())}
        # STRONG scaling of the sweep (north_star: ">= 6x further at 8 GPUs on a 512-restart acquisition sweep"): the total number of restarts fixed, sharded
        # r % P over the ranks, at 512 and at 8192 restarts; time = max over ranks (device sampler: the same draw whatever P is)
        strong = {}
        for total in (512, 8192):
            kw = dict(num_restarts=total, raw_samples=4 * total, device_rand=True, builtin_constraint=True)
            run_sweep(device, **kw)
            run_sweep(device, **kw)                  # (two warm-ups, as for the latency table below: 8192 restarts is the first use of the generic-workspace kernels)
            if dist is not None:
                dist.barrier()
            best_s, best_v, best_log = float("inf"), None, {}
            for _ in range(5):
                s_, _, v_, log_ = run_sweep(device, **kw)
                if s_ < best_s:
                    best_s, best_v, best_log = s_, v_, log_
            ts_ = torch.tensor([best_s], dtype=torch.float64, device=device)
            fl_ = torch.tensor([1.0 if best_log.get("native_sweep") else 0.0, 1.0 if best_log.get("device_selection") else 0.0], dtype=torch.float64, device=device)
            coll_s = 0.0
            if dist is not None:
                dist.all_reduce(ts_, op=dist.ReduceOp.MAX)
                dist.all_reduce(fl_, op=dist.ReduceOp.MIN)
                # the two collectives of a sharded sweep on their own (same shapes: the raw-row table, the result rows), max over ranks
                from gabotorch_amd.manifold_optimization.manifold_optimize import _all_gather_rows
                per_, rper_ = (4 * total + world - 1) // world, (total + world - 1) // world
                tab_, res_ = torch.zeros(world * (per_ + 1), 16, dtype=torch.float64, device=device), torch.zeros(world * rper_, 17, dtype=torch.float64, device=device)
                for rep_ in range(4):
                    torch.cuda.synchronize()
                    dist.barrier()
                    t0_ = time.perf_counter()
                    _all_gather_rows(dist, tab_, tab_[:per_ + 1].clone())
                    _all_gather_rows(dist, res_, res_[:rper_].clone())
                    res_.cpu()
                    coll_s = time.perf_counter() - t0_
                tc_ = torch.tensor([coll_s], dtype=torch.float64, device=device)
                dist.all_reduce(tc_, op=dist.ReduceOp.MAX)
                coll_s = float(tc_.item())
            strong[str(total)] = {"restarts": total, "raw_samples": 4 * total, "n_gpus": world, "seconds": float(ts_.item()),
                                  "restarts_per_s": total / float(ts_.item()), "best_acq": best_v,
                                  "native_sweep_on_every_rank": bool(fl_[0].item() > 0), "selection_on_the_device_on_every_rank": bool(fl_[1].item() > 0),
                                  "seconds_of_the_two_collectives_alone": coll_s}
        # one GPU: the sweep's latency as a function of the number of restarts IT holds, which is what a rank of a P-GPU run sees (R / P restarts):
        # predicted strong-scaling speed-up S_P(R) = t_1(R) / t_1(R / P), the all_gather of R x 16 doubles (< 20 us over xGMI) neglected
        latency_table = None
        if world == 1 and not lite:
            latency_table = {}
            for total in (64, 128, 256, 1024, 2048, 4096, 16384, 32768, 65536):
                kw = dict(num_restarts=total, raw_samples=4 * total, device_rand=True, builtin_constraint=True)
                try:
                    run_sweep(device, **kw)
                    run_sweep(device, **kw)          # (two warm-ups: a new size means new workspaces and, beyond 1024 restarts, other kernel variants)
                    latency_table[total] = min(run_sweep(device, **kw)[0] for _ in range(3))
                except Exception as err:       # noqa: BLE001  (a size the maximiser declines must not take the headline line with it)
                    print(f"sweep with {total} restarts failed: {err}", file=sys.stderr)
            latency_table[512], latency_table[8192] = strong["512"]["seconds"], strong["8192"]["seconds"]
            latency_table = {str(k): latency_table[k] for k in sorted(latency_table)}
        # the two forms of the single-launch solve side by side (gabo_spd_tr_two_waves): one wave per restart, and two - the second evaluating the
        # proposal truncated CG is about to make while the first evaluates the finite-difference point; bit-identical results
        two_waves = None
        if world == 1 and not lite:
            import ctypes
            from gabotorch_amd import _lib as _gl
            lib_ = _gl.load()
            two_waves = {}
            before_ = lib_.gabo_spd_tr_two_waves(-1)
            try:
                for total in (64, 512):
                    kw = dict(num_restarts=total, raw_samples=4 * total, device_rand=True, builtin_constraint=True)
                    row = {}
                    for name_, flag_ in (("one_wave", 0), ("two_waves", 1)):
                        lib_.gabo_spd_tr_two_waves(flag_)
                        run_sweep(device, **kw)
                        h_, m_ = ctypes.c_longlong(0), ctypes.c_longlong(0)
                        lib_.gabo_spd_tr_two_waves_counters(ctypes.byref(h_), ctypes.byref(m_), 1)
                        runs_ = [run_sweep(device, **kw) for _ in range(5)]
                        lib_.gabo_spd_tr_two_waves_counters(ctypes.byref(h_), ctypes.byref(m_), 1)
                        row["seconds_" + name_] = min(r_[0] for r_ in runs_)
                        row["best_acq_" + name_] = runs_[0][2]
                        if flag_:
                            row["iterations_with_the_speculated_step"] = h_.value // 5
                            row["iterations_without"] = m_.value // 5
                    two_waves[str(total)] = row
            finally:
                lib_.gabo_spd_tr_two_waves(before_)
        sweep = {"workload": "gabo_spd S^5_++: GP(50 obs of the Ackley objective, SURVEY 8d)+EI, 2048 raw samples, 512 restarts, ConstrainedTR semantics, FD Hessian, "
                             "lambda_max<=5 constraint built with functools.partial as in the reference example; raw samples drawn in one "
                             "vectorised host call and scored by the fused chain; the trust-region solve is ONE launch (every wave iterates "
                             "its restart: tCG, proposal, acquisition, constraint, update); restarts sharded over ranks, all_gather+argmax",
                 "seconds": float(tt.item()), "restarts_per_s": 512 / float(tt.item()), "best_acq": sw_val,
                 "tr_iterations": int(sw_log["iterations"]),
                 "seconds_constraint_as_opaque_lambda_hipgraphs": sw_l,
                 "seconds_constraints_captured": sw_c, "best_acq_constraints_captured": sw_val_c,
                 "seconds_constraints_captured_device_rand": sw_d, "best_acq_device_rand": sw_val_d,
                 "seconds_single_launch_solve": sw_s, "seconds_single_launch_solve_device_rand": sw_sd, "best_acq_single_launch_solve": sw_val_s,
                 "best_acq_single_launch_solve_device_rand": sw_val_sd,
                 "seconds_single_launch_solve_device_rand_python_path": sw_sd_py, "best_acq_single_launch_solve_device_rand_python_path": sw_val_sd_py,
                 "native_host_driver": "the device-sampled sweep runs through the native driver (csrc/spd_sweep.hip): gabo_spd_gp_prepare (one host call for the GP's "
                                       "set-up), then gabo_spd_sweep_score_rows -> gabo_spd_sweep_select_rows (botorch's initialize_q_batch_nonneg as a kernel on the "
                                       "library's Philox stream) -> gabo_spd_sweep_solve_rows (a start launch and the solve, which ends with the result rows): five launches and "
                                       "one host wait; with the selection left on the host (options['device_selection'] = False) it returns the Python path's candidate "
                                       "bit for bit, with the selection on the device the Python path returns the same candidate when handed the kernel's picks "
                                       "(tests/test_gpu_native_sweep.py); with several ranks the SAME driver runs on every rank (two all_gathers on its two tables)",
                 "weak_scaling_512_restarts_per_gpu": weak,
                 "strong_scaling_fixed_total_restarts": strong,
                 "seconds_by_restarts_one_gpu": latency_table,
                 "single_launch_solve_one_and_two_waves_per_restart": two_waves,
                 "note": "latency-bound: a restart walks its trust-region iterations serially.  Up to 512 restarts the solve launch gives every restart TWO waves "
                         "(csrc/spd_tr_duo_body.hpp): truncated CG almost always leaves in its first step through the trust-region boundary, a step that does not depend "
                         "on the Hessian-vector product, so the second wave builds and evaluates that proposal while the first evaluates the finite-difference point "
                         "(an accepted iteration ~82 k cycles instead of ~138 k when the speculation holds, the one-wave schedule when it does not; bit-identical "
                         "results, tests/test_gpu_two_waves.py); runs of rejected proposals whose first tCG step does not change (a restart outside an eigenvalue "
                         "bound: 98 iterations, formerly the duration of the launch) are applied as scalar updates.  Solve launch at 64 restarts 0.70 -> 0.49 ms.  Round 6 "
                         "also removed what surrounded it: per-GP set-up in one host call (gp_factor 104 -> 62 us, hidden behind the host's set-up), ten launches in front of the solve "
                         "and three behind it folded into one start launch and the solve launch, the selection heuristic on the device (no host wait between scoring and solving), scores / picks / results "
                         "in page-locked memory the kernels address directly.  Does not speed up with more GPUs at this size (see expected_scaling)"}



    sphere_sweep_result = None
    if args.full and not args.no_sweep:
        # the sphere counterpart of the sweep (gabo_sphere's setting: stock trust regions with EXACT Hessian-vector products, no
        # constraints): GP(50 obs) + EI on S^9, 512 restarts sharded over the ranks - one launch for the whole solve (csrc/sphere_tr.hip).
        # Every rank takes part: the maximiser broadcasts / all_gathers when torch.distributed is initialised.
        from tools.sphere_sweep_bench import run as sphere_sweep
        sphere_sweep(approx=False, constrained=False, device=device)
        if dist is not None:
            dist.barrier()
        ssw = min(sphere_sweep(approx=False, constrained=False, device=device)[0] for _ in range(3))
        sval = sphere_sweep(approx=False, constrained=False, device=device)[1]
        tsw = torch.tensor([ssw], dtype=torch.float64, device=device)
        if dist is not None:
            dist.all_reduce(tsw, op=dist.ReduceOp.MAX)
        ssw = float(tsw.item())
        s_dev = s_host_sel = s_dev_val = None
        if dist is None and not args.sweep_lite:
            sphere_sweep(approx=False, constrained=False, device=device, device_rand=True)
            s_dev = min(sphere_sweep(approx=False, constrained=False, device=device, device_rand=True)[0] for _ in range(3))
            s_dev_val = sphere_sweep(approx=False, constrained=False, device=device, device_rand=True)[1]
            s_host_sel = min(sphere_sweep(approx=False, constrained=False, device=device, device_selection=False)[0] for _ in range(3))
        sphere_sweep_result = {"workload": "SphereGaussianKernel GP(50 obs)+EI on S^9, 2048 raw samples, 512 restarts, stock trust regions "
                                           "with exact Hessian-vector products (closed form on the device); one process: ONE host call with one wait "
                                           "(gabo_sphere_sweep_run: scoring, restart selection as a kernel, start, single-launch solve, arg-max), raw samples "
                                           "from the host sampler",
                               "seconds": ssw, "restarts_per_s": 512 / ssw, "best_acq": sval,
                               "seconds_raw_samples_drawn_on_the_device": s_dev, "best_acq_raw_samples_drawn_on_the_device": s_dev_val,
                               "seconds_two_calls_selection_on_the_host": s_host_sel,
                               "note": "round 6: the evaluations' triangular loops with lane-dependent bounds became dense unrolled matrix-vector products on "
                                       "the symmetric inverse, the solve keeps A, the training points and its workspace in LDS (solve launch 869 -> 240 us), the "
                                       "selection moved to the device (one host wait instead of two): 1.69 -> 0.84 ms, 0.61 with the device sampler"}

    t = torch.tensor([wall], dtype=torch.float64, device=device)
    if dist is not None:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    wall_max = float(t.item())
    pairs_per_step = N_POINTS * N_POINTS
    value = world * pairs_per_step * args.steps / wall_max

    if rank == 0:
        parity = None
        if args.full:
            # correctness gate inside the bench: a 256 x 256 block against the oracle
            from oracle import spd as ospd
            blk = job.out[:256, :256].cpu().numpy()
            want = ospd.spd_ai_gaussian_kernel(x[:256], x[:256], BETA)
            max_rel = float(np.max(np.abs(blk - want) / np.abs(want)))
            max_rel_sym = 0.0
            if sym is not None:
                sym_blk = sym.out[:256, :256].cpu().numpy()
                max_rel_sym = float(np.max(np.abs(sym_blk - want) / np.abs(want)))
            if not (max_rel < 1e-5 and max_rel_sym < 1e-5):
                raise RuntimeError(f"parity gate failed: {max_rel} {max_rel_sym}")
            parity = {"max_rel_err_vs_oracle_256x256": max_rel, "symmetric": max_rel_sym, "tolerance": 1e-5}
        kernel_s = ev_ms * 1e-3               # prep + pairwise launches; the pairwise kernel is > 99.5 % of it (profiles/)
        ach_gbs = pairs_per_step * BYTES_PER_PAIR / kernel_s / 1e9
        ach_tf = pairs_per_step * FLOP_PER_PAIR / kernel_s / 1e12
        traffic, traffic_source = None, None
        if (args.traffic == "measure" or (args.traffic == "auto" and args.full)) and world == 1:
            traffic, traffic_source = measure_hbm_traffic()
            if traffic is None and args.traffic == "measure":
                raise RuntimeError(f"--traffic measure: {traffic_source}")
        pmc = os.path.join(ROOT, "profiles", "pmc_summary.json")
        if traffic is None and os.path.exists(pmc):
            traffic = json.load(open(pmc)).get("hbm_bytes_per_launch")
            traffic_source = ("profiles/pmc_summary.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of the same launch, committed; NOT re-measured "
                              f"inside this run: {traffic_source or 'not requested'})")
        line = {
            "metric": "SPD affine-invariant kernel-matrix build, pairs/sec (N=4096,d=10)",
            "value": value, "unit": "pairs/s", "n_gpus": world, "world_size": world, "backend": backend, "steps": args.steps, "warmup": args.warmup,
            "untimed_preheat_steps": max(args.preheat, 0),
            "ms_per_step": wall_max / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": "SpdAffineInvariantGaussianKernel S^10_++ Gram K(X,X), N=4096 random SPD 10x10 (Mandel, "
                                   "eig U[0.05,5], seed 1234+rank), beta=0.2+ln2, all N^2 pairs evaluated; one independent "
                                   "point set per GPU", "n_points": N_POINTS, "dim": DIM, "parallelism": f"independent Gram builds x{world}"},
            "roofline": {"bound": "mfma", "bound_note": "the harness token for 'compute-bound'; what binds is the fp64 VECTOR issue rate - the kernel issues no MFMA "
                                                        "instruction (PMC SQ_INSTS_VALU_MFMA_MOPS_F64 = 0) and the f64 matrix pipe shares the datapath",
                         "mfma_instructions": 0,
                         "binding_resource": "fp64 issue (vector pipe; the f64 matrix pipe shares it: tools/ubench_mfma_f64.hip)",
                         "achieved": ach_tf, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": ach_tf / FP64_PEAK_TFLOPS,
                         "traffic": traffic, "traffic_source": traffic_source,
                         "traffic_over_compulsory": None if traffic is None else traffic / (pairs_per_step * 8.0 + 2 * N_POINTS * (DIM * (DIM + 1) // 2) * 8),
                         "kernel": "gabo::spd_ai_pairwise_kernel<10>", "kernel_ms": ev_ms,
                         "kernel_ms_median": float(np.median(step_ms)), "kernel_ms_min": float(np.min(step_ms)),
                         "frac_at_median": pairs_per_step * FLOP_PER_PAIR / (float(np.median(step_ms)) * 1e-3) / 1e12 / FP64_PEAK_TFLOPS,
                         "model": f"{FLOP_PER_PAIR:.0f} algorithmic flop/pair (SURVEY 8d: congruence + tridiagonalisation + QL) x {pairs_per_step} "
                                  "pairs per launch / launch duration (HIP events on the launch stream over the timed steps); fp64 vector = matrix "
                                  "peak 78.6 TFLOP/s",
                         "measured_sustained_v_fma_f64": 60.6, "measured_sustained_mfma_f64": 77.8},
            "roofline_hbm_streaming_model": {"non_physical": True, "achieved": ach_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                             "frac": ach_gbs / HBM_PEAK_GBS,
                                             "model": f"SURVEY 8(d) streaming model: {BYTES_PER_PAIR} B/pair (both d x d tiles charged to every pair). "
                                                      "The operands are L2-resident and never re-fetched from HBM, so this figure can exceed 1 and is "
                                                      "not evidence of bandwidth use; the measured HBM traffic is `roofline.traffic`"},
            "symmetric_gram": None if sym is None else {
                "ms_per_step": sym_ms, "pairs_per_s": pairs_per_step / (sym_ms * 1e-3),
                "note": "x1 is x2 shortcut (GABO_SYMMETRIC): i <= j evaluated, mirrored; not used for `value`"},
            "parity": parity, "full": args.full,
        }
        line["expected_scaling"] = {
            "note": "stated BEFORE any multi-GPU hardware run (none was available to the builder): the model a SCALE run is to be judged against",
            "value_independent_gram_builds": "P x the 1-GPU value: one point set and one launch stream per rank, no data-path collective "
                                             "(only the two barriers around the timed region)",
            "sharded_gram.left_sharded": "strong, ~P: t(P) = t_prep(N points on every rank, 6 us) + t_pairwise(1 GPU)/P; at P = 8: 2.4/8 + 0.01 = 0.31 ms "
                                         "(the N/P x N row block is 512 x 4096 pairs = 512 wave-rows per 64 columns: still > 4 waves per SIMD)",
            "sharded_gram.all_gathered": "strong, ~3x at P = 8: each rank receives (P-1)/P of the 134 MB result, 16.8 MB from each of 7 peers over its own "
                                         "xGMI link (76.8 GB/s per direction peak, ~50 GB/s assumed): 0.34 ms on top of the 0.31 ms of compute; leave the "
                                         "Gram sharded when the consumer is sharded",
            "acq_sweep.strong_512_restarts": "~1.1-1.2x at P = 8 before the two collectives (see acq_sweep.strong_measured_model for this run's table): a restart is ONE "
                                             "wave that runs ~12 accepted trust-region iterations of ~58 us serially, one GPU holds 512 such waves at one per SIMD with room to "
                                             "spare, so a rank with 64 restarts finishes barely earlier than one GPU with all 512. north_star's >= 6x at 8 GPUs is NOT reachable for "
                                             "a sweep of this size with a wave-per-restart solver (it is from ~16 384 restarts); what rounds 5-6 did instead is cut the one-GPU "
                                             "time of this sweep 3.8x (4.2-4.6 -> 1.5 -> 1.15-1.18 ms) and make every rank of a sharded sweep run the native driver",
            "acq_sweep.weak_scaling_512_restarts_per_gpu": "~P x restarts/s: per-rank work unchanged, one all_gather of (value, sample) rows for the raw samples "
                                                           "(2048 x 16 doubles per rank) and one of (value, candidate) per restart (512 x 16 doubles per rank)",
            "measured_single_gpu_latencies_us": {"tr_iteration_launch_64_restarts": 86, "tr_iteration_launch_512_restarts": 113,
                                                 "tr_iteration_launch_2048_restarts": 182, "tr_iteration_launch_8192_restarts": 597}}
        if sweep is not None and sweep.get("seconds_by_restarts_one_gpu"):
            tab = {int(k): v for k, v in sweep["seconds_by_restarts_one_gpu"].items()}
            pred = {str(r): tab[r] / tab[r // 8] for r in sorted(tab) if r // 8 in tab}
            reach = [r for r in sorted(tab) if r // 8 in tab and tab[r] / tab[r // 8] >= 6.0]
            line["expected_scaling"]["acq_sweep.strong_measured_model"] = {
                "model": "S_8(R) = t_1(R) / t_1(R / 8) from THIS run's one-GPU sweep times (device sampler, single-launch solve; `acq_sweep.seconds_by_restarts_one_gpu`); "
                         "a rank of an 8-GPU run holds R / 8 restarts and R / 2 raw samples; the all_gather of the R candidate rows is < 20 us",
                "predicted_speedup_at_8_gpus_by_total_restarts": pred,
                "smallest_total_restarts_reaching_6x_at_8_gpus": reach[0] if reach else None,
                "north_star_512_restarts": f"predicted {pred.get('512', float('nan')):.2f}x at 8 GPUs: the 512-restart sweep is latency-bound (one wave per restart, "
                                           "2 waves per CU on one GPU already), so the >= 6x of north_star is reached only from the restart count above"}
        if plugin is not None:
            line["plugin_surface"] = plugin
            line["forward_ms"] = {"no_grad": plugin["spd"]["forward_ms_no_grad"], "grad_enabled": plugin["spd"]["forward_ms_grad_enabled"],
                                  "no_grad_x_is_x": plugin["spd"]["forward_ms_no_grad_x_is_x"], "sphere_no_grad": plugin["sphere"]["forward_ms_no_grad"],
                                  "sphere_grad_enabled": plugin["sphere"]["forward_ms_grad_enabled"],
                                  "what": "SpdAffineInvariantGaussianKernel.forward / SphereGaussianKernel.forward at N = 4096 (details: plugin_surface)"}
        if collectives is not None:
            line["collectives"] = collectives
        if sweep is not None:
            line["acq_sweep"] = sweep
        if sharded is not None:
            line["sharded_gram"] = sharded
        if sphere_sweep_result is not None:
            line["acq_sweep_sphere"] = sphere_sweep_result
        if args.full and not args.no_sweep and not args.sweep_lite:
            # config 2 of BASELINE.json beside the headline: SphereGaussianKernel S^9, N=4096 (HBM-write bound: 8.04 B/pair)
            from gabotorch_amd import ops as _ops
            from oracle import sphere as osph
            srng = np.random.default_rng(1234)
            sx = srng.standard_normal((N_POINTS, 10))
            sx /= np.linalg.norm(sx, axis=1, keepdims=True)
            st_ = torch.tensor(sx, device=device)
            sbeta = 0.6 + float(np.log(2.0))
            # On a stream of its own: while the hipGraph executables of the sweeps above are alive, every launch on the process's DEFAULT
            # stream pays for its implicit ordering against their streams - this write-bound kernel 42 instead of 31 us, back to 31 on any
            # other stream or once the graphs are destroyed (tools/sphere_bench_probe5.py).  The headline job ran before any graph existed.
            import gc
            gc.collect()

            def cold20():
                """what a caller who builds ONE Gram sees: launches 1..20 after a device synchronisation, each between its own pair of events"""
                torch.cuda.synchronize()
                ev_ = [torch.cuda.Event(enable_timing=True) for _ in range(21)]
                ev_[0].record()
                for c_ in range(20):
                    _ops.sphere_pairwise(st_, st_, beta=sbeta)
                    ev_[c_ + 1].record()
                torch.cuda.synchronize()
                return [ev_[c_].elapsed_time(ev_[c_ + 1]) for c_ in range(20)]
            sph_cold_default = cold20()          # on the process's default stream (with the sweeps' hipGraph executables alive: see above)
            sph_stream = torch.cuda.Stream(device)
            sph_stream.wait_stream(torch.cuda.current_stream(device))
            _sph_ctx = torch.cuda.stream(sph_stream)
            _sph_ctx.__enter__()
            # Untimed launches first, as for the headline kernel.  This kernel is bound by the HBM write stream, and the chip's clock / power
            # management needs ~450 back-to-back launches (15 ms) of it to settle: per block of 50 launches 33, 40, 41, 38, 37, 36, 35, 35, 33,
            # 32, 32, 31 us (tools/sphere_bench_probe3.py; 30.4-30.8 us over 2000 launches, tools/sphere_bench_probe.py) - after a phase
            # without memory traffic (the fp64 Gram builds and latency-bound sweeps above) even more.  Timed: five blocks of 100 launches,
            # the median block reported, all five disclosed.
            sph_preheat, sph_block, sph_blocks = 600, 100, 5
            sph_cold = cold20()
            for _ in range(sph_preheat):
                _ops.sphere_pairwise(st_, st_, beta=sbeta)
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(sph_blocks + 1)]
            evs[0].record()
            for blk in range(sph_blocks):
                for _ in range(sph_block):
                    ks = _ops.sphere_pairwise(st_, st_, beta=sbeta)
                evs[blk + 1].record()
            torch.cuda.synchronize()
            sph_block_ms = [evs[b_].elapsed_time(evs[b_ + 1]) / sph_block for b_ in range(sph_blocks)]
            sph_ms = float(np.median(sph_block_ms))
            sph_err = float(np.max(np.abs(ks[:128, 4000:].cpu().numpy() - osph.sphere_gaussian_kernel(sx[:128], sx[4000:], sbeta))))
            _sph_ctx.__exit__(None, None, None)
            torch.cuda.current_stream(device).wait_stream(sph_stream)
            line["sphere_gram"] = {"workload": "SphereGaussianKernel S^9 Gram, N=4096 (BASELINE config 2)", "ms_per_step": sph_ms,
                                   "pairs_per_s": pairs_per_step / (sph_ms * 1e-3),
                                   "roofline": {"bound": "hbm", "achieved": pairs_per_step * 8.04 / (sph_ms * 1e-3) / 1e9,
                                                "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                                "frac": pairs_per_step * 8.04 / (sph_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                                "model": "8.04 algorithmic B/pair (one fp64 output + amortised operand reads)"},
                                   "cold_ms": float(np.median(sph_cold_default)), "cold_ms_first_launch": sph_cold_default[0],
                                   "cold_ms_private_stream": float(np.median(sph_cold)),
                                   "cold_note": "median / first of launches 1-20 after a device synchronisation, no preheat, each launch between its own pair of "
                                                "events (the launch gap is inside): `cold_ms` on the default stream, `cold_ms_private_stream` on the stream the "
                                                "sustained figure is taken on",
                                   "untimed_preheat_launches": sph_preheat, "timed": f"{sph_blocks} blocks of {sph_block} launches, median block, on a non-default stream",
                                   "ms_per_step_of_each_block": sph_block_ms, "max_abs_err_vs_oracle_block": sph_err}
            line["roofline_sphere"] = dict(line["sphere_gram"]["roofline"], kernel="gabo::sphere_pairwise_kernel<0, true, 3, false, false, true>", kernel_ms=sph_ms,
                                           binding_resource="the HBM write stream (MFMA + stores alone: 26 us; the epilogue reads the kernel value from a "
                                                            "per-launch table: no exp per output) + 3 us of table-building prologue without stores in flight")
            with torch.cuda.stream(sph_stream):          # (same reason: the write-bound Gram kernels of config 5)
                line["config5"] = config5_pieces(device)
                line["hd_sphere"] = hd_sphere_pieces(device)
            torch.cuda.current_stream(device).wait_stream(sph_stream)
            # the step before the sweep in a BO iteration: surrogate fit (fit_gpytorch_model), 50 observations on S^5_++
            import time as _time
            from gabotorch_amd import models as _models
            from gabotorch_amd._compat import ScaleKernel as _Scale
            from gabotorch_amd.kernel_utils.kernels_spd import SpdAffineInvariantGaussianKernel as _AiKernel
            fx_ = torch.tensor(synthetic_spd_mandel(50, 5, 99), device=device)
            fy_ = torch.tensor(np.random.default_rng(99).standard_normal(50), device=device)
            fit_ms = {}
            for label, fast in (("one_launch_per_evaluation", True), ("autograd_through_the_kernels", False)):
                best_t = float("inf")
                for _ in range(3):
                    gp_ = _models.SingleTaskGP(fx_, fy_, _Scale(_AiKernel(beta_min=0.25), outputscale_prior=_models.GammaPrior(2.0, 0.15)),
                                               noise_prior=_models.GammaPrior(1.1, 0.05))
                    torch.cuda.synchronize()
                    t0_ = _time.perf_counter()
                    _models.fit_gpytorch_model(gp_, fast=fast)
                    torch.cuda.synchronize()
                    best_t = min(best_t, _time.perf_counter() - t0_)
                fit_ms[label] = best_t * 1e3
            # the closed-form backward of the headline kernel on the headline workload (every GP fit by autograd and every generic-path
            # acquisition gradient pays it): d/dx1 of sum(G o K), all N^2 pairs, HIP events on the launch stream
            from gabotorch_amd import ops as _bops
            xb_ = torch.tensor(np.ascontiguousarray(x), device=device)
            gb_ = torch.ones(N_POINTS, N_POINTS, dtype=torch.float64, device=device)
            for _ in range(3):
                _bops.spd_ai_backward(xb_, xb_, gb_, BETA)
            bev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
            bev[0].record()
            for b_ in range(5):
                gx_ = _bops.spd_ai_backward(xb_, xb_, gb_, BETA)
                bev[b_ + 1].record()
            torch.cuda.synchronize()
            bwd_ms = float(np.median([bev[b_].elapsed_time(bev[b_ + 1]) for b_ in range(5)]))
            from oracle import spd as _ospd
            ga_, _ = _ospd.spd_ai_gaussian_kernel_grads(x[:24], x, BETA, np.ones((24, N_POINTS)))
            bwd_err = float(np.max(np.abs(gx_[:24].cpu().numpy() - ga_)) / np.max(np.abs(ga_)))
            d3 = float(DIM) ** 3
            bwd_flop = (4.0 / 3.0 + 4.0 / 3.0 + 6.0 + 1.0 + 2.0 / 3.0) * d3
            line["spd_backward"] = {"workload": "gabo_spd_ai_backward: d/dx1 of sum(G o K) on the headline Gram (N=4096, d=10, all N^2 pairs)", "ms": bwd_ms,
                                    "pairs_per_s": pairs_per_step / (bwd_ms * 1e-3), "ratio_to_forward": bwd_ms / ev_ms,
                                    "max_rel_err_vs_oracle_first_24_rows": bwd_err}
            line["roofline_backward"] = {"bound": "mfma", "bound_note": "compute-bound on the fp64 VECTOR pipe like the forward (no MFMA instruction)", "mfma_instructions": 0,
                                         "achieved": pairs_per_step * bwd_flop / (bwd_ms * 1e-3) / 1e12, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s",
                                         "frac": pairs_per_step * bwd_flop / (bwd_ms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS,
                                         "kernel": "gabo::spd_ai_backward_kernel<10>", "kernel_ms": bwd_ms,
                                         "model": f"{bwd_flop:.0f} algorithmic flop/pair = (2/3 congruence + 4/3 tridiagonalisation + 4/3 accumulation of the reflectors + ~6 "
                                                  "implicit QL with eigenvectors at two sweeps per eigenvalue + 1 for V log(L) V^T) d^3, the LAPACK dsyev operation count "
                                                  "plus the matrix function; x N^2 pairs / launch duration (HIP events, median of 5)"}
            if not (bwd_err < 1e-9):
                raise RuntimeError(f"backward parity gate failed: {bwd_err}")
            line["surrogate_fit"] = {"workload": "fit_gpytorch_model: SingleTaskGP(ScaleKernel(SpdAffineInvariantGaussianKernel)), 50 "
                                                 "observations on S^5_++, Gamma priors, L-BFGS-B (gabo_gp_mll: likelihood + analytic "
                                                 "gradient in one launch per evaluation)", "ms": fit_ms}
        if args.full and world == 1 and not args.no_cpu_baseline:
            cb, kcpu = cpu_baseline(x)
            cb["max_rel_diff_gpu_vs_cpu_port"] = float(np.max(np.abs(job.out[:kcpu.shape[0]].cpu().numpy() - kcpu) / np.abs(kcpu)))
            line["cpu_baseline"] = cb
        print(json.dumps(line))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
