"""Times the point preconditioners and simple! on the device CSC of fdrand(n,n,n) (default 256^3): Jacobi and ILU0 ldiv!
on device vectors, update! values-only, the first build after a pattern change (create), and one simple! step with ILU0
(averaged over --iters steps).  The library runs on torch's current stream (esp_set_stream), so device events bracket its
work; every call also returns synchronised.  Prints one JSON line: ms and the algorithmic bytes of DESIGN.md.

    python tools/precon_bench.py [--n 256] [--iters 50] [--warmup 5]

--kind iluam times ILUAMPreconditioner instead: the first build (analysis + factorization), a values-only update!, ldiv! on
device vectors, one simple! step, and the number of kernel launches of one ldiv! (computed from the level sizes of the
stencil cube by the library's grouping rule; the kernel trace of DESIGN.md section 5e counts the same).  --tol-n M adds
simple! to reltol = 1e-8 on fdrand(M,M,M), b = ones, with ILU0 and with ILUAM: iterations and wall time of each.
--cpu-model adds the host time of the sequential reference loops (tests/iluam_model.c) at the same size.

    python tools/precon_bench.py --kind iluam [--n 256] [--iters 10] [--tol-n 40] [--cpu-model]

--kind cg times preconditioned conjugate gradients (esp_cg): for Identity, Jacobi, ILU0 and ILUAM the time of one CG iteration
(a run of --iters + 1 iterations minus a run of 1, reltol = 0) and, from the same process, one simple! step of the same
preconditioner measured twice (its run-to-run spread); then iterations and wall time to reltol = 1e-8 with b = ones at --n
and at --tol-n.  --cg-only NAME restricts it to one preconditioner and skips simple! and the solves (what a kernel trace wants:
rocprofv3 --kernel-trace --stats -- python tools/precon_bench.py --kind cg --cg-only ilu0 --iters 20 --warmup 0).

    python tools/precon_bench.py --kind cg [--n 256] [--iters 20] [--tol-n 40] [--tol-maxiter 20000]

--kind bicgstabl times BiCGStab(l) (esp_bicgstabl): for Identity, Jacobi, ILU0 and ILUAM and l = 1, 2, 4 (--ls) the time of one
OUTER iteration (2l matrix-vector products; a run of --iters + 1 outer iterations minus a run of 1, reltol = 0), measured twice,
and beside it the same statements composed from what the package offered before esp_bicgstabl -- A.mul, P.ldiv, torch vector
operations, torch.dot and torch.linalg.solve on device tensors, the scalars kept on the device, one read-back per outer iteration:
what a user would have written --, measured twice in the same process (the two alternate), and the ratio composed / fused.  --cg-only NAME
restricts it to one preconditioner, --no-composed leaves the composition out (what a kernel trace wants).

    python tools/precon_bench.py --kind bicgstabl [--n 256] [--iters 5] [--ls 1,2,4] [--cg-only ilu0] [--no-composed]

--kind gmres times restarted GMRES (esp_gmres): for Identity, Jacobi and ILU0 (--cg-only NAME: one of them) and orth_meth mgs and
dgks (--orths), restart 20, the time of two full cycles (maxiter = 40, reltol = 0) and beside it composed_gmres, the same statements
composed from what the package offered before esp_gmres -- A.mul, P.ldiv, torch vector operations, the scalars kept on the device,
one read-back per iteration (two with DGKS: its decision), the small least-squares problem on the host --, in --rounds alternating
rounds of the same call; it first asserts that the two histories agree to 1e-10 relative.  Reported: every round's time, the
medians, the spread of the fused rounds (max - min: the margin of "the fused solve is no slower"), and the time of iteration
k = 1, 10 and 20 of the first cycle (a run of k iterations minus a run of k - 1; k = 1 carries the first solution update).
--kind gmres-trace is what a kernel trace wants: ONE solve of two full cycles with one preconditioner (--cg-only, default jacobi)
and the first orth_meth of --orths, on device vectors.

    python tools/precon_bench.py --kind gmres [--n 256] [--rounds 5] [--orths mgs,dgks] [--cg-only ilu0] [--no-composed]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- \
        python tools/precon_bench.py --kind gmres-trace --cg-only jacobi --orths mgs --n 256

--kind block times BlockPreconditioner (esp_precon_block_create) against the unblocked preconditioner of the same kind, for Jacobi,
ILU0 and ILUAM (--cg-only NAME: one of them): create, the values-only update! and ldiv! on device vectors for (a) the unblocked
preconditioner, (b) odd / even unknowns, (c) 8 and (d) 64 contiguous slabs (identity path), (e) a seeded random permutation in 8
parts (permuted path).  All five stay alive and are timed in --rounds alternating rounds of --iters warm calls each; reported: the
median over the rounds, every round's value, and for ldiv! the unblocked kind's spread over the rounds (max - min), the yardstick of
"identity-path ldiv! takes no more than the unblocked one".  ILUAM's level counts are listed for each.

    python tools/precon_bench.py --kind block [--n 256] [--iters 20] [--rounds 5] [--cg-only ilu0]

--kind block-trace is what a kernel trace wants: one preconditioner (--cg-only NAME, --block-config a..e), a create and --iters
ldiv! calls on device vectors (--iters 0: the create alone; the difference of two traces is the kernel list of ldiv!).
--kind block-trace-diff --dirs WITH WITHOUT [--iters K] reads the two traces' *_kernel_stats.csv / *_memory_copy_stats.csv and prints the
kernels and copies per ldiv! call.

    rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d OUT -- \
        python tools/precon_bench.py --kind block-trace --cg-only ilu0 --block-config b --n 64 --iters 25 --warmup 0

--kind amg times AMGPreconditioner (esp_precon_amg_create) on fdrand(n,n,n): the setup (create; then update!, which rebuilds the
whole hierarchy, --rounds times: median, min, max), ldiv! on device vectors (--rounds rounds of --iters calls each: median, min,
max), the level sizes, the operator complexity (the stored entries of all A_l over those of A_0) and the Luby rounds of every
level, and cg to reltol = 1e-8 with b = ones with AMG and with ILU0: iterations and wall time of each (the second of two solves).

--coarsen rs times RS_AMGPreconditioner (esp_precon_rsamg_create, Ruge-Stueben coarsening) the same way; "luby_rounds" are then
the rounds of the PMIS splitting.  It adds gmres(restart = 20) to reltol = 1e-8 with RS and with ILU0 on the upwind
convection-diffusion matrix of tests/bicgstabl_modellib.py at --cd-n cubed unknowns and Peclet number --cd-pe (b = ones).

    python tools/precon_bench.py --kind amg [--coarsen sa|rs] [--n 64] [--iters 20] [--rounds 5] [--tol-maxiter 20000]

--kind iluk --k K times ILUKPreconditioner (esp_precon_iluk_create) on fdrand(n,n,n) beside ILUAMPreconditioner, the yardstick, in the
same run: the create (median over --rounds of create + close; the ILUAM analysis + factorization part is timed on a copy of B, the
search + sort part is the rest), a values-only update!, ldiv!, nnz(B)/nnz(A), the three ILUAM level counts, the counters of the search,
and gmres(restart = 20) / cg to reltol 1e-8 on b = ones (iterations and time).

    python tools/precon_bench.py --kind iluk --k 1 [--n 64] [--iters 20] [--rounds 5]

--kind colored [--inner ilu0|iluam] times ColoredPreconditioner (esp_precon_colored_create, the multicolour ordering) on fdrand(n,n,n)
beside the natural-order ILUAMPreconditioner and ILU0Preconditioner, the yardsticks, in the same run: the create (median over
--rounds of create + close) with the colouring's share split off (esp_graph_coloring alone: its rounds are the colours), a values-only
update!, ldiv! on device vectors, the colours and the level counts, and cg to reltol 1e-8 on b = ones (iterations and time).

    python tools/precon_bench.py --kind colored --inner iluam [--n 64] [--iters 20] [--rounds 5]

--kind spai0 | spai1 | spai1sym times SPAIPreconditioner (esp_precon_spai_create: SPAI-0, SPAI-1, the symmetrised SPAI-1) on
fdrand(n,n,n): setup_ms (create), update_ms (values-only update!), ldiv_ms beside mul_ms (one mul! of A) and cg to 1e-8, with Jacobi,
ILU0 and ColoredPreconditioner (--inner) from the same run beside it.

    python tools/precon_bench.py --kind spai1sym [--n 64] [--iters 20] [--rounds 5] [--tol-maxiter 20000]

--kind ilut [--droptol T --steps S --sweeps W] times ILUTPreconditioner (esp_precon_ilut_create) on fdrand(n,n,n) beside ILU0, ILUAM
and ILU(1) from the same run, the creates alternated round by round: set-up (create), update (update! without keep_pattern: the
construction again), warm update (keep_pattern: the sweeps alone) and one sweep (the difference of two warm updates that differ by
four sweeps, beside the bytes the sweep must move at least), nnz(F)/nnz(A), the level counts, ldiv!, and cg / gmres(restart = 20) to
reltol 1e-8 on b = ones (iterations and time).

    python tools/precon_bench.py --kind ilut --droptol 1e-2 [--n 64] [--iters 20] [--rounds 5] [--tol-maxiter 20000]

--kind lu [--leaf-size L] times LUFactorization (esp_precon_lu_create) on fdrand(n,n,n): the create and its parts (the ordering alone
through esp_nested_dissection, ILUAM's analysis + factorization of a copy of B, the fill as what is left), a values-only update!,
ldiv!, nnz(B)/nnz(A), the rounds and launches of the ordering, ILUAM's level counts, and one solve of A x = 1 to 1e-8: A.solve(b)
(create + solve) against cg with ILU0 and with ILUAM (create + cg) in the same run.  Medians over --rounds.
    python tools/precon_bench.py --kind lu [--n 32] [--leaf-size 32] [--iters 5] [--rounds 5]
--kind lu --form both | panels times the forms of LUFactorization side by side in alternating rounds in one process (both: the column
form, the yardstick, and the panel form; panels: the panel form alone), CholeskyFactorization and cg with ILU0 beside them:
    python tools/precon_bench.py --kind lu --form both [--n 24] [--leaf-size 32] [--iters 5] [--rounds 5]
--kind cholesky [--leaf-size L] [--lu-rounds R] times CholeskyFactorization (esp_precon_cholesky_create) on fdrand(n,n,n) beside
LUFactorization, the yardstick, in the same process and the same alternating rounds (LU in the first R of them): the ordering alone,
the create, a values-only update! and ldiv! on device vectors; every round's value, medians, spreads (max - min), the ratios, the launch
counts, nnz(L), the panel bytes, the residual for b = ones, and cg with ILU0 to 1e-8 from the same run.
    python tools/precon_bench.py --kind cholesky [--n 24] [--lu-rounds 5] [--iters 5] [--rounds 5]
--nrhs K[,K...] with --kind cholesky, --kind lu --form columns|panels, --kind iluam, --kind colored or --kind mul times several right-hand sides in one call
(esp_precon_ldiv_many / esp_mul_many) against K single-vector calls of the same build in the same process, on device
arrays: alternating rounds of --iters repetitions each; every round's value, medians, spreads (max - min), the time per column and
the ratio K singles / one call.  It first asserts that the columns of the two agree bit for bit.
    python tools/precon_bench.py --kind cholesky --nrhs 1,8,32 [--n 32] [--iters 3] [--rounds 5]
    python tools/precon_bench.py --kind lu --form panels --nrhs 1,8,32 [--n 32]
    python tools/precon_bench.py --kind mul --nrhs 1,8,32 [--n 128] [--iters 10]
    python tools/precon_bench.py --kind iluam --nrhs 1,8,32 [--n 128]      (ILUAMPreconditioner: iluam_solve_many)
    python tools/precon_bench.py --kind colored --nrhs 1,8,32 [--n 128]    (ColoredPreconditioner over ILUAM)
--nrhs K[,K...] with --kind cg [--cg-only identity|jacobi|ilu0|iluam] times cg(A, B) with K columns in one call (esp_cg_many, DESIGN.md
5u) against K single cg calls of the same build in the same process, on fdrand(n,n,n) and device arrays, random right-hand sides, the
default tolerance and at most --iters iterations a solve: one solve of each per alternating round; every round's value, medians,
spreads (max - min), the time per column, the ratio K singles / one call and the iteration counts.  It first asserts that x, the
history, the iteration count and the flag of every column agree bit for bit.
    python tools/precon_bench.py --kind cg --cg-only ilu0 --nrhs 1,8,32 [--n 128] [--iters 50] [--rounds 5]
--nrhs K[,K...] with --kind gmres [--cg-only identity|jacobi|ilu0|iluam] [--restart 20] [--orth mgs|cgs|dgks] times gmres(A, B) with
K columns in one call (esp_gmres_many) against K single gmres calls in the same way; reltol = 0 and --iters iterations
a solve, so every column takes all of them.  It first asserts that x, the history, the three counters and the flag of every column
agree bit for bit.
    python tools/precon_bench.py --kind gmres --cg-only ilu0 --nrhs 1,8,32 --iters 40 [--n 128] [--restart 20] [--orth mgs]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cube_level_sizes(n):
    """members of the levels of fdrand(n,n,n)'s three schedules: the nodes (i,j,k) with i + j + k = l"""
    import numpy as np
    one = np.ones(n, np.int64)
    return np.convolve(np.convolve(one, one), one)


def grouped_launches(sizes, wg=256):
    """the library's rule (iluam.hip, build_schedule): a level wider than a workgroup is a launch of its own, consecutive
    levels that together fit one workgroup share one"""
    launches, room = 0, 0
    for c in sizes:
        if c > wg:
            launches, room = launches + 1, 0
        elif c <= room:
            room -= c
        else:
            launches, room = launches + 1, wg - c
    return launches


def bench_iluam(a, torch, esp):
    import numpy as np
    A = esp.fdrand(a.n, a.n, a.n)
    d = A._d
    stream = torch.cuda.current_stream()
    d.ck(d.lib.esp_set_stream(d.h, C.c_void_p(stream.cuda_stream)))
    N, Z = A.n, A.nnz()
    v = torch.randn(N, dtype=torch.float64, device="cuda")
    u = torch.empty_like(v)
    b = torch.ones_like(v)

    def timed(fn, reps, warmup=a.warmup):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    out = {"workload": "iluam_fdrand", "n": a.n, "N": N, "nnz": Z}
    Pw = esp.ILU0Preconditioner(A)     # builds the row-wise index esp_mul shares, so that the build below is ILUAM's own
    Pw.close()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    P = esp.ILUAMPreconditioner(A)     # first build: row parts, three level analyses, numeric factorization
    e1.record()
    e1.synchronize()
    out["iluam_create_ms"] = e0.elapsed_time(e1)
    out["levels"] = list(P.levels())
    out["iluam_update_values_ms"] = timed(lambda: P.update(), max(3, a.iters // 3), warmup=1)
    assert list(P.levels()) == out["levels"]
    out["iluam_ldiv_ms"] = timed(lambda: P.ldiv(v, out=u), a.iters)

    def run_simple(k):
        x = torch.zeros_like(v)
        esp.simple(A, b, u=x, Pl=P, maxiter=k, reltol=0.0)

    t_long = timed(lambda: run_simple(a.iters + 1), 2, warmup=1)
    t_short = timed(lambda: run_simple(1), 2, warmup=1)
    out["simple_iluam_step_ms"] = (t_long - t_short) / a.iters
    sizes = cube_level_sizes(a.n)
    assert len(sizes) == out["levels"][1]
    out["ldiv_launches"] = 2 * grouped_launches(sizes)      # forward + backward (the backward sizes are the mirror image)
    out["factor_launches"] = grouped_launches(sizes)
    if a.cpu_model:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import tempfile
        from iluam_modellib import Model
        arrays = tuple(np.array(x, copy=True) for x in A.sparse().arrays())
        with tempfile.TemporaryDirectory() as td:
            M = Model(td)
            t0 = time.perf_counter()
            f, dg = M.factor(arrays)
            out["cpu_model_factor_ms"] = (time.perf_counter() - t0) * 1e3
            hv = v.cpu().numpy()
            t0 = time.perf_counter()
            M.ldiv(arrays, f, dg, hv)
            out["cpu_model_ldiv_ms"] = (time.perf_counter() - t0) * 1e3
    P.close()
    if a.tol_n:
        m = a.tol_n
        B = esp.fdrand(m, m, m)
        ones = torch.ones(B.n, dtype=torch.float64, device="cuda")
        for name, cls in (("ilu0", esp.ILU0Preconditioner), ("iluam", esp.ILUAMPreconditioner)):
            Q = cls(B)
            esp.simple(B, ones, Pl=Q, maxiter=3, reltol=0.0)   # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, log = esp.simple(B, ones, Pl=Q, maxiter=a.tol_maxiter, reltol=1e-8, log=True)
            dt = time.perf_counter() - t0                       # (esp_simple returns synchronised)
            r = log["resnorm"]
            out["tol_%s" % name] = {"n": m, "iterations": len(r) - 1, "converged": bool(r[-1] / r[0] < 1e-8), "ms": dt * 1e3}
            Q.close()
    print(json.dumps({k: (round(x, 4) if isinstance(x, float) else x) for k, x in out.items()}))


def bench_cg(a, torch, esp):
    A = esp.fdrand(a.n, a.n, a.n)
    d = A._d
    stream = torch.cuda.current_stream()
    d.ck(d.lib.esp_set_stream(d.h, C.c_void_p(stream.cuda_stream)))
    N, Z = A.n, A.nnz()
    b = torch.ones(N, dtype=torch.float64, device="cuda")
    kinds = {"identity": lambda M: None, "jacobi": esp.JacobiPreconditioner, "ilu0": esp.ILU0Preconditioner,
             "iluam": esp.ILUAMPreconditioner}
    names = [a.cg_only] if a.cg_only else list(kinds)

    def timed(fn, reps):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def per_step(run):
        """ms of one iteration: a run of iters + 1 minus a run of 1 (both include the start-up and the zeroed vector)"""
        return (timed(lambda: run(a.iters + 1), 2) - timed(lambda: run(1), 2)) / a.iters

    out = {"workload": "cg_fdrand", "n": a.n, "N": N, "nnz": Z, "iters": a.iters}
    # what one CG iteration moves beyond the ldiv! and the mul! of a simple! step: u = c + beta*u (3 N doubles), x += alpha*u and
    # r -= alpha*c (6 N), r read once more by the preconditioner's dot product (N)
    out["extra_vector_GB"] = round(8 * 10 * N / 1e9, 3)
    for name in names:
        P = kinds[name](A)
        rec = {}
        rec["cg_iteration_ms"] = per_step(lambda k: esp.cg(A, b, Pl=P, maxiter=k, reltol=0.0))
        if P is not None and not a.cg_only:
            step = lambda k: esp.simple(A, b, u=torch.zeros_like(b), Pl=P, maxiter=k, reltol=0.0)
            rec["simple_step_ms"] = [per_step(step), per_step(step)]
        if not a.cg_only:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x, log = esp.cg(A, b, Pl=P, maxiter=a.tol_maxiter, reltol=1e-8, log=True)
            dt = time.perf_counter() - t0                   # (esp_cg returns synchronised)
            true = torch.linalg.vector_norm(b - A.mul(x)).item()
            last = log["resnorm"][-1] if log["iters"] else log["r0"]
            rec["tol"] = {"n": a.n, "iterations": log["iters"], "converged": log["isconverged"], "ms": dt * 1e3,
                          "true_over_recurrence": true / last}
        if P is not None:
            P.close()
        out[name] = rec
    if a.tol_n and not a.cg_only:
        m = a.tol_n
        B = esp.fdrand(m, m, m)
        ones = torch.ones(B.n, dtype=torch.float64, device="cuda")
        for name in names:
            Q = kinds[name](B)
            esp.cg(B, ones, Pl=Q, maxiter=3, reltol=0.0)   # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, log = esp.cg(B, ones, Pl=Q, maxiter=a.tol_maxiter, reltol=1e-8, log=True)
            dt = time.perf_counter() - t0
            out[name]["tol_small"] = {"n": m, "iterations": log["iters"], "converged": log["isconverged"], "ms": dt * 1e3}
            if Q is not None:
                Q.close()

    def rnd(x):
        if isinstance(x, float):
            return round(x, 4)
        if isinstance(x, dict):
            return {k: rnd(y) for k, y in x.items()}
        if isinstance(x, list):
            return [rnd(y) for y in x]
        return x

    print(json.dumps(rnd(out)))


def composed_bicgstabl(torch, A, P, b, l, outer):
    """the statements of esp_bicgstabl (include/esparse_hip.h) from the package's parts: `outer` outer iterations from x = 0"""
    ldiv = (lambda v, out: P.ldiv(v, out=out)) if P is not None else (lambda v, out: out.copy_(v))
    rs = [torch.zeros_like(b) for _ in range(l + 1)]
    us = [torch.zeros_like(b) for _ in range(l + 1)]
    x = torch.zeros_like(b)
    t = torch.empty_like(b)
    ldiv(b, rs[0])
    rt = rs[0].clone()
    omega = sigma = torch.ones((), dtype=torch.float64, device=b.device)
    hist = [torch.linalg.vector_norm(rs[0]).item()]
    for _ in range(outer):
        sigma = -omega * sigma
        for j in range(l):
            rho = torch.dot(rt, rs[j])
            beta = rho / sigma
            for k in range(j + 1):
                torch.sub(rs[k], us[k] * beta, out=us[k])
            ldiv(A.mul(us[j], out=t), us[j + 1])
            sigma = torch.dot(rt, us[j + 1])
            alpha = rho / sigma
            for k in range(j + 1):
                rs[k].sub_(us[k + 1] * alpha)
            ldiv(A.mul(rs[j], out=t), rs[j + 1])
            x.add_(us[0] * alpha)
        R = torch.stack(rs)
        M = R @ R.T
        gamma = torch.linalg.solve(M[1:, 1:], M[1:, 0])
        for k in range(1, l + 1):
            us[0].sub_(us[k] * gamma[k - 1])
        for k in range(1, l + 1):
            x.add_(rs[k - 1] * gamma[k - 1])
        for k in range(1, l + 1):
            rs[0].sub_(rs[k] * gamma[k - 1])
        omega = gamma[l - 1]
        hist.append(torch.linalg.vector_norm(rs[0]).item())   # the stop test's read-back
    return x, hist


def bench_bicgstabl(a, torch, esp):
    A = esp.fdrand(a.n, a.n, a.n)
    d = A._d
    stream = torch.cuda.current_stream()
    d.ck(d.lib.esp_set_stream(d.h, C.c_void_p(stream.cuda_stream)))
    N, Z = A.n, A.nnz()
    b = torch.ones(N, dtype=torch.float64, device="cuda")
    kinds = {"identity": lambda M: None, "jacobi": esp.JacobiPreconditioner, "ilu0": esp.ILU0Preconditioner,
             "iluam": esp.ILUAMPreconditioner}
    names = [a.cg_only] if a.cg_only else list(kinds)
    ls = [int(v) for v in a.ls.split(",")]

    def timed(fn, reps):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def per_outer(run):
        """ms of one outer iteration: a run of iters + 1 minus a run of 1 (both include the start-up and the zeroed vectors)"""
        return (timed(lambda: run(a.iters + 1), 2) - timed(lambda: run(1), 2)) / a.iters

    out = {"workload": "bicgstabl_fdrand", "n": a.n, "N": N, "nnz": Z, "iters": a.iters}
    for name in names:
        P = kinds[name](A)
        rec = {}
        for l in ls:
            fused = lambda k: esp.bicgstabl(A, b, l=l, Pl=P, max_mv_products=2 * l * k, reltol=0.0)
            if a.no_composed:
                r = {"fused_outer_ms": [per_outer(fused), per_outer(fused)]}
            else:   # the two alternate: fused, composed, fused, composed
                comp = lambda k: composed_bicgstabl(torch, A, P, b, l, k)
                t = [per_outer(fused), per_outer(comp), per_outer(fused), per_outer(comp)]
                r = {"fused_outer_ms": t[0::2], "composed_outer_ms": t[1::2]}
                r["composed_over_fused"] = min(r["composed_outer_ms"]) / min(r["fused_outer_ms"])
                # the two run the same statements: their histories agree to the rounding of the sums
                _, log = esp.bicgstabl(A, b, l=l, Pl=P, max_mv_products=4 * l, reltol=0.0, log=True)
                _, hist = composed_bicgstabl(torch, A, P, b, l, 2)
                r["history_rel_diff"] = max(abs(g - w) / w for g, w in zip([log["r0"]] + list(log["resnorm"]), hist))
            rec["l%d" % l] = r
        if P is not None:
            P.close()
        out[name] = rec

    def rnd(x):
        if isinstance(x, float):
            return float("%.4g" % x)
        if isinstance(x, dict):
            return {k: rnd(y) for k, y in x.items()}
        if isinstance(x, list):
            return [rnd(y) for y in x]
        return x

    print(json.dumps(rnd(out)))


def composed_gmres(torch, A, P, b, restart, maxiter, orth):
    """the statements of esp_gmres (include/esparse_hip.h) from the package's parts: `maxiter` iterations from x = 0, reltol = 0"""
    import numpy as np
    ldiv = (lambda v, out: P.ldiv(v, out=out)) if P is not None else (lambda v, out: out.copy_(v))
    n = b.numel()
    V = torch.empty((restart + 1, n), dtype=torch.float64, device=b.device)
    H = torch.zeros((restart + 1, restart), dtype=torch.float64, device=b.device)
    x = torch.zeros_like(b)
    t = torch.empty_like(b)
    eta = 1.0 / np.sqrt(2.0)
    ldiv(b, V[0])
    beta = torch.linalg.vector_norm(V[0])
    V[0].div_(beta)
    hist = [beta.item()]
    it = 0
    while it < maxiter:
        nullvec = torch.ones(restart + 1, dtype=torch.float64, device=b.device)
        acc = torch.ones((), dtype=torch.float64, device=b.device)
        k = 0
        while k < restart and it < maxiter:
            w = V[k + 1]
            ldiv(A.mul(V[k], out=t), w)
            if orth == "mgs":
                for i in range(k + 1):
                    h = torch.dot(V[i], w)
                    H[i, k] = h
                    w.sub_(V[i] * h)
                nrm = torch.linalg.vector_norm(w)
            else:
                h = V[:k + 1] @ w
                w.sub_(h @ V[:k + 1])
                nrm = torch.linalg.vector_norm(w)
                if orth == "dgks":
                    proj, passes = torch.linalg.vector_norm(h), 0
                    while passes < 3 and bool(nrm < eta * proj):   # the decision's read-back
                        c = V[:k + 1] @ w
                        proj = torch.linalg.vector_norm(c)
                        w.sub_(c @ V[:k + 1])
                        h = h + c
                        nrm = torch.linalg.vector_norm(w)
                        passes += 1
                H[:k + 1, k] = h
            H[k + 1, k] = nrm
            w.div_(nrm)
            nv = -(torch.dot(nullvec[:k + 1], H[:k + 1, k]) / nrm)
            nullvec[k + 1] = nv
            acc = acc + nv * nv
            hist.append((beta / torch.sqrt(acc)).item())   # the stop test's read-back
            k += 1
            it += 1
        Hh = H[:k + 1, :k].cpu().numpy()                   # the small least-squares problem on the host
        e1 = np.zeros(k + 1)
        e1[0] = beta.item()
        y = np.linalg.lstsq(Hh, e1, rcond=None)[0]
        x.add_(torch.from_numpy(y).to(b.device) @ V[:k])
        if it < maxiter:
            torch.sub(b, A.mul(x, out=t), out=t)
            ldiv(t, V[0])
            beta = torch.linalg.vector_norm(V[0])
            V[0].div_(beta)
    return x, hist


def bench_gmres(a, torch, esp):
    import statistics
    A = esp.fdrand(a.n, a.n, a.n)
    d = A._d
    stream = torch.cuda.current_stream()
    d.ck(d.lib.esp_set_stream(d.h, C.c_void_p(stream.cuda_stream)))
    N, Z = A.n, A.nnz()
    b = torch.ones(N, dtype=torch.float64, device="cuda")
    kinds = {"identity": lambda M: None, "jacobi": esp.JacobiPreconditioner, "ilu0": esp.ILU0Preconditioner}
    names = [a.cg_only] if a.cg_only else list(kinds)
    restart, maxiter = 20, 40

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    out = {"workload": "gmres_fdrand", "n": a.n, "N": N, "nnz": Z, "restart": restart, "maxiter": maxiter, "rounds": a.rounds}
    for name in names:
        P = kinds[name](A)
        rec = {}
        for orth in a.orths.split(","):
            fused = lambda k=maxiter: esp.gmres(A, b, Pl=P, restart=restart, maxiter=k, reltol=0.0, orth_meth=orth, log=True)
            comp = lambda: composed_gmres(torch, A, P, b, restart, maxiter, orth)
            r = {}
            _, log = fused()                                   # (also the warm-up: the work space is sized here)
            r["reorth"] = log["reorth"]
            if not a.no_composed:
                _, hist = comp()
                got = [log["r0"]] + list(log["resnorm"])
                r["history_rel_diff"] = max(abs(g - w) / w for g, w in zip(got, hist))
                assert len(got) == len(hist) == maxiter + 1 and r["history_rel_diff"] <= 1e-10, r
            tf, tc = [], []
            for _ in range(a.rounds):                          # the two alternate
                tf.append(timed(fused))
                if not a.no_composed:
                    tc.append(timed(comp))
            r["fused_ms"], r["fused_median_ms"], r["fused_spread_ms"] = tf, statistics.median(tf), max(tf) - min(tf)
            if tc:
                r["composed_ms"], r["composed_median_ms"] = tc, statistics.median(tc)
                r["composed_over_fused"] = r["composed_median_ms"] / r["fused_median_ms"]
                r["fused_no_slower"] = r["fused_median_ms"] <= r["composed_median_ms"] + r["fused_spread_ms"]
            run = {k: min(timed(lambda: fused(k)) for _ in range(3)) for k in (0, 1, 9, 10, 19, 20)}
            r["iteration_ms"] = {"k1": run[1] - run[0], "k10": run[10] - run[9], "k20": run[20] - run[19]}
            rec[orth] = r
        if P is not None:
            P.close()
        out[name] = rec

    def rnd(x):
        if isinstance(x, float):
            return float("%.4g" % x)
        if isinstance(x, dict):
            return {k: rnd(y) for k, y in x.items()}
        if isinstance(x, list):
            return [rnd(y) for y in x]
        return x

    print(json.dumps(rnd(out)))


def bench_gmres_trace(a, torch, esp):
    """what a kernel trace wants: ONE solve of two full cycles (restart 20, maxiter 40, reltol 0) on device vectors with one
    preconditioner (--cg-only, default jacobi) and one orth_meth (the first of --orths)"""
    A = esp.fdrand(a.n, a.n, a.n)
    b = torch.ones(A.n, dtype=torch.float64, device="cuda")
    name, orth = a.cg_only or "jacobi", a.orths.split(",")[0]
    P = {"identity": lambda M: None, "jacobi": esp.JacobiPreconditioner, "ilu0": esp.ILU0Preconditioner,
         "iluam": esp.ILUAMPreconditioner}[name](A)
    _, log = esp.gmres(A, b, Pl=P, restart=20, maxiter=40, reltol=0.0, orth_meth=orth, log=True)
    print(json.dumps({"workload": "gmres_trace", "n": a.n, "precon": name, "orth_meth": orth, "iters": log["iters"],
                      "mvps": log["mvps"], "reorth": log["reorth"]}))
    if P is not None:
        P.close()


def block_partitioning(np, N, config):
    """1-based partitions of 1..N for the configurations b .. e of --kind block"""
    if config == "b":
        return [np.arange(1, N + 1, 2), np.arange(2, N + 1, 2)]
    if config in ("c", "d"):
        k = 8 if config == "c" else 64
        cuts = [(N * i) // k for i in range(k + 1)]
        return [np.arange(cuts[i] + 1, cuts[i + 1] + 1) for i in range(k)]
    perm = np.random.default_rng(15).permutation(N) + 1
    cuts = [(N * i) // 8 for i in range(9)]
    return [perm[cuts[i]:cuts[i + 1]] for i in range(8)]


def make_block(esp, np, A, cls, config):
    return cls(A) if config == "a" else esp.BlockPreconditioner(A, block_partitioning(np, A.n, config), cls)


def bench_block(a, torch, esp):
    import statistics

    import numpy as np
    A = esp.fdrand(a.n, a.n, a.n)
    d = A._d
    stream = torch.cuda.current_stream()
    d.ck(d.lib.esp_set_stream(d.h, C.c_void_p(stream.cuda_stream)))
    N, Z = A.n, A.nnz()
    v = torch.randn(N, dtype=torch.float64, device="cuda")
    u = torch.empty_like(v)
    kinds = {"jacobi": esp.JacobiPreconditioner, "ilu0": esp.ILU0Preconditioner, "iluam": esp.ILUAMPreconditioner}
    names = [a.cg_only] if a.cg_only else list(kinds)
    configs = ["a", "b", "c", "d", "e"]
    labels = {"a": "unblocked", "b": "odd_even", "c": "slabs8", "d": "slabs64", "e": "random8_permuted"}

    def timed(fn, reps, warmup):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    out = {"workload": "block_precon_fdrand", "n": a.n, "N": N, "nnz": Z, "iters": a.iters, "rounds": a.rounds}
    Pw = esp.ILU0Preconditioner(A)     # builds A's row-wise index once, so that no create below pays for it
    Pw.close()
    for name in names:
        rec, P = {}, {}
        print("block bench: %s" % name, file=sys.stderr, flush=True)
        for c in configs:
            parts = None if c == "a" else block_partitioning(np, N, c)   # (the host-side index arrays are not part of create)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            P[c] = kinds[name](A) if c == "a" else esp.BlockPreconditioner(A, parts, kinds[name])
            r = {"create_ms": (time.perf_counter() - t0) * 1e3}             # (create returns synchronised; the partition upload included)
            if c != "a":
                r["path"] = P[c].path
                b, _ = P[c]._block()
                z = C.c_int64()
                d.ck(d.lib.esp_nnz(b, C.byref(z)))
                r["nnz_B"] = z.value
            if name == "iluam":
                r["levels"] = list(P[c].levels())
            rec[labels[c]] = r
        upd = {c: [] for c in configs}
        ldv = {c: [] for c in configs}
        for rnd_i in range(a.rounds):                                       # the five alternate inside every round
            for c in configs:
                ldv[c].append(timed(lambda: P[c].ldiv(v, out=u), a.iters, a.warmup if rnd_i == 0 else 1))
            for c in configs:
                upd[c].append(timed(lambda: P[c].update(), max(2, a.iters // 5), 1))
        for c in configs:
            r = rec[labels[c]]
            r["ldiv_ms"], r["ldiv_rounds_ms"] = statistics.median(ldv[c]), ldv[c]
            r["update_values_ms"], r["update_rounds_ms"] = statistics.median(upd[c]), upd[c]
        spread = max(ldv["a"]) - min(ldv["a"])
        rec["unblocked_ldiv_spread_ms"] = spread
        rec["identity_within_unblocked_plus_spread"] = {labels[c]: bool(rec[labels[c]]["ldiv_ms"] <= rec["unblocked"]["ldiv_ms"] + spread)
                                                        for c in ("b", "c", "d")}
        for c in configs:
            P[c].close()
        out[name] = rec

    def rnd(x):
        if isinstance(x, float):
            return float("%.5g" % x)
        if isinstance(x, dict):
            return {k: rnd(y) for k, y in x.items()}
        if isinstance(x, list):
            return [rnd(y) for y in x]
        return x

    print(json.dumps(rnd(out)))


def bench_block_trace(a, torch, esp):
    import numpy as np
    A = esp.fdrand(a.n, a.n, a.n)
    d = A._d
    d.ck(d.lib.esp_set_stream(d.h, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    v = torch.randn(A.n, dtype=torch.float64, device="cuda")
    u = torch.empty_like(v)
    cls = {"jacobi": esp.JacobiPreconditioner, "ilu0": esp.ILU0Preconditioner, "iluam": esp.ILUAMPreconditioner}[a.cg_only or "ilu0"]
    P = make_block(esp, np, A, cls, a.block_config)
    torch.cuda.synchronize()
    for _ in range(a.iters):
        P.ldiv(v, out=u)
    torch.cuda.synchronize()
    print(json.dumps({"workload": "block_trace", "n": a.n, "kind": a.cg_only or "ilu0", "config": a.block_config, "ldiv_calls": a.iters,
                      "path": getattr(P, "path", None)}))
    P.close()


def block_trace_diff(a):
    """kernels and copies per ldiv! call: the trace of create + K ldiv! minus the trace of the create alone"""
    import csv
    import glob

    def counts(d, what):
        """calls per name: from the --stats table (Name, Calls) where there is one, else the rows of the trace"""
        c = {}
        stats = glob.glob(os.path.join(d, "**", "*_%s_stats.csv" % what), recursive=True)
        col = "Kernel_Name" if what == "kernel" else "Direction"
        for f in stats or glob.glob(os.path.join(d, "**", "*_%s_trace.csv" % what), recursive=True):
            with open(f, newline="") as fh:
                for row in csv.DictReader(fh):
                    key = row["Name"] if stats else row.get(col, "?")
                    c[key] = c.get(key, 0) + (int(row["Calls"]) if stats else 1)
        return c

    with_d, without_d = a.dirs
    out = {"ldiv_calls": a.iters}
    for what, src in (("kernels_per_ldiv", "kernel"), ("copies_per_ldiv", "memory_copy")):
        w, wo = counts(with_d, src), counts(without_d, src)
        out[what] = {k: (w.get(k, 0) - wo.get(k, 0)) / a.iters for k in sorted(set(w) | set(wo)) if w.get(k, 0) != wo.get(k, 0)}
    print(json.dumps(out))


def bench_amg(a, torch, esp):
    import statistics
    A = esp.fdrand(a.n, a.n, a.n)
    d = A._d
    stream = torch.cuda.current_stream()
    d.ck(d.lib.esp_set_stream(d.h, C.c_void_p(stream.cuda_stream)))
    N, Z = A.n, A.nnz()
    v = torch.randn(N, dtype=torch.float64, device="cuda")
    u = torch.empty_like(v)
    b = torch.ones_like(v)

    def span(fn, reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def stats(xs):
        return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": len(xs)}

    cls = esp.RS_AMGPreconditioner if a.coarsen == "rs" else esp.AMGPreconditioner
    out = {"workload": "amg_fdrand", "coarsen": a.coarsen, "n": a.n, "N": N, "nnz": Z}
    t0 = time.perf_counter()
    P = cls(A)                                        # the first build (the level handles' indices included)
    out["create_first_ms"] = (time.perf_counter() - t0) * 1e3
    note = lambda: print(json.dumps(out), file=sys.stderr, flush=True)   # (what is known so far, should a later phase be cut short)
    note()
    out["setup_ms"] = stats([span(P.update, 1) for _ in range(max(a.rounds, 1))])
    lib, p = d.lib, P._p
    sizes, nnzs, rounds = [], [], []
    for l in range(P.levels):
        ha, n, rho, rd, z = C.c_void_p(), C.c_int64(), C.c_double(), C.c_int32(), C.c_int64()
        d.ck(lib.esp_precon_amg_level(p, l, C.byref(ha), None, C.byref(n), C.byref(rho), C.byref(rd)))
        d.ck(lib.esp_nnz(ha, C.byref(z)))
        sizes.append(n.value), nnzs.append(z.value), rounds.append(rd.value)
    out["level_sizes"], out["level_nnz"], out["luby_rounds"] = sizes, nnzs, rounds
    out["operator_complexity"] = sum(nnzs) / max(nnzs[0], 1)
    note()
    for _ in range(a.warmup):
        P.ldiv(v, out=u)
    out["ldiv_ms"] = stats([span(lambda: P.ldiv(v, out=u), a.iters) for _ in range(max(a.rounds, 1))])
    note()
    Q = esp.ILU0Preconditioner(A)
    for name, pl in (("amg", P), ("ilu0", Q)):
        rec = None
        for _ in range(2):                            # (the first solve sizes the work vectors)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x, log = esp.cg(A, b, Pl=pl, maxiter=a.tol_maxiter, reltol=1e-8, log=True)
            dt = time.perf_counter() - t0             # (esp_cg returns synchronised)
            rec = {"iterations": log["iters"], "converged": log["isconverged"], "ms": dt * 1e3}
        rec["true_residual_over_b"] = (torch.linalg.vector_norm(b - A.mul(x)) / torch.linalg.vector_norm(b)).item()
        out["cg_" + name] = rec
        note()
    P.close()
    Q.close()
    if a.coarsen == "rs" and a.cd_n > 0:              # a non-symmetric M-matrix: gmres with RS against ILU0
        import numpy as np
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from bicgstabl_modellib import convdiff_triplets
        m = a.cd_n
        I, J, V = convdiff_triplets(m, m, m, a.cd_pe)
        B = esp.ExtendableSparseMatrix(m ** 3, m ** 3)
        B.append(esp.ESP_UPDATE, I, J, V)
        B.flush()
        ones = torch.ones(B.n, dtype=torch.float64, device="cuda")
        rec = {"n": m, "pe": a.cd_pe, "N": B.n, "nnz": B.nnz(), "restart": 20}
        for name, kind in (("rs", esp.RS_AMGPreconditioner), ("ilu0", esp.ILU0Preconditioner)):
            t0 = time.perf_counter()
            pl = kind(B)
            r = {"create_ms": (time.perf_counter() - t0) * 1e3}
            if name == "rs":
                r["levels"] = pl.levels
            for _ in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                x, log = esp.gmres(B, ones, Pl=pl, restart=20, maxiter=a.tol_maxiter, reltol=1e-8, log=True)
                dt = time.perf_counter() - t0         # (esp_gmres returns synchronised)
                r.update({"iterations": log["iters"], "converged": log["isconverged"], "ms": dt * 1e3})
            r["true_residual_over_b"] = (torch.linalg.vector_norm(ones - B.mul(x)) / np.sqrt(B.n)).item()
            rec[name] = r
            pl.close()
        out["gmres_convdiff"] = rec

    def rnd(x):
        if isinstance(x, float):
            return float("%.5g" % x)
        if isinstance(x, dict):
            return {k: rnd(y) for k, y in x.items()}
        if isinstance(x, list):
            return [rnd(y) for y in x]
        return x

    print(json.dumps(rnd(out)))


def bench_iluk(a, torch, esp):
    import numpy as np
    A = esp.fdrand(a.n, a.n, a.n)
    d = A._d
    stream = torch.cuda.current_stream()
    d.ck(d.lib.esp_set_stream(d.h, C.c_void_p(stream.cuda_stream)))
    N, Z = A.n, A.nnz()
    v = torch.randn(N, dtype=torch.float64, device="cuda")
    u = torch.empty_like(v)
    b = torch.ones_like(v)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()                                   # (create, update!, ldiv! and the solvers return synchronised)
        return (time.perf_counter() - t0) * 1e3, r

    def median(xs):
        return float(np.median(xs))

    def measure(make, M=A):
        rec = {}
        ts = []
        for _ in range(a.rounds):
            t, P = wall(lambda: make(M))
            ts.append(t)
            P.close()
        rec["create_ms"] = median(ts)
        P = make(M)
        rec["update_values_ms"] = median([wall(P.update)[0] for _ in range(a.rounds)])
        for _ in range(3):
            P.ldiv(v, out=u)
        rec["ldiv_ms"] = median([wall(lambda: [P.ldiv(v, out=u) for _ in range(a.iters)])[0] / a.iters for _ in range(a.rounds)])
        rec["levels"] = list(P.levels())
        return rec, P

    def solvers(rec, P):
        for name, fn in (("gmres", lambda: esp.gmres(A, b, Pl=P, restart=20, reltol=1e-8, maxiter=a.tol_maxiter, log=True)),
                         ("cg", lambda: esp.cg(A, b, Pl=P, reltol=1e-8, maxiter=a.tol_maxiter, log=True))):
            fn()
            ts, log = [], None
            for _ in range(a.rounds):
                t, (_, log) = wall(fn)
                ts.append(t)
            rec[name] = {"iterations": log["iters"], "converged": log["isconverged"], "ms": median(ts)}

    out = {"workload": "iluk_fdrand", "n": a.n, "N": N, "nnz": Z, "k": a.k, "rounds": a.rounds}
    Pw = esp.ILU0Preconditioner(A)     # builds the row-wise index esp_mul shares, so that the creates below are their own
    Pw.close()
    rec, P = measure(esp.ILUAMPreconditioner)
    solvers(rec, P)
    P.close()
    out["iluam"] = rec
    rec, P = measure(lambda M: esp.ILUKPreconditioner(M, a.k))
    st = P.stats()
    rec["nnz_B"] = st["nnz"]
    rec["fill_ratio"] = st["nnz"] / Z
    rec["stats"] = st
    solvers(rec, P)
    cp, rv, nz = P.fill_matrix()
    P.close()
    Bm = esp.ExtendableSparseMatrix(esp.SparseMatrixCSC(N, N, cp, rv, nz))      # ILUAM's analysis + factorization of B, on a copy
    Bm.flush()
    Pw = esp.ILU0Preconditioner(Bm)
    Pw.close()
    ts = []
    for _ in range(a.rounds):
        t, Q = wall(lambda: esp.ILUAMPreconditioner(Bm))
        ts.append(t)
        Q.close()
    rec["create_iluam_of_B_ms"] = median(ts)
    rec["create_search_sort_ms"] = rec["create_ms"] - rec["create_iluam_of_B_ms"]
    out["iluk"] = rec

    def rnd(x):
        if isinstance(x, float):
            return round(x, 4)
        if isinstance(x, dict):
            return {k: rnd(y) for k, y in x.items()}
        return x
    print(json.dumps(rnd(out)))


def bench_lu(a, torch, esp):
    """LUFactorization on fdrand n^3: the create split into ordering / fill / ILUAM's analysis + factorization of B, the values-only
    update, ldiv!, the fill, the rounds and launches of the ordering, ILUAM's level counts, and one solve to 1e-8 -- A.solve(b)
    against cg with ILU0 and with ILUAM in the same run.  Medians over --rounds."""
    import numpy as np
    A = esp.fdrand(a.n, a.n, a.n)
    d = A._d
    stream = torch.cuda.current_stream()
    d.ck(d.lib.esp_set_stream(d.h, C.c_void_p(stream.cuda_stream)))
    N, Z = A.n, A.nnz()
    v = torch.randn(N, dtype=torch.float64, device="cuda")
    u = torch.empty_like(v)
    b = torch.ones_like(v)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()                                   # (create, update!, ldiv! and the solvers return synchronised)
        return (time.perf_counter() - t0) * 1e3, r

    def median(xs):
        return float(np.median(xs))

    out = {"workload": "lu_fdrand", "n": a.n, "N": N, "nnz": Z, "leaf_size": a.leaf_size, "rounds": a.rounds}
    Pw = esp.ILU0Preconditioner(A)     # builds the row-wise index the ordering shares, so that the creates below are their own
    Pw.close()
    rec = {}

    def note(what):                                # (a phase is done: a line on stderr, so that a run cut short still reports)
        print("lu n=%d: %s: %s" % (a.n, what, json.dumps({k: v for k, v in rec.items() if k != "stats"})), file=sys.stderr, flush=True)
    rec["ordering_ms"] = median([wall(lambda: esp.nested_dissection(A, a.leaf_size))[0] for _ in range(a.rounds)])
    ts = []
    for _ in range(a.rounds):
        t, P = wall(lambda: esp.LUFactorization(A, a.leaf_size))
        ts.append(t)
        P.close()
    rec["create_ms"] = median(ts)
    note("create")
    P = esp.LUFactorization(A, a.leaf_size)
    st = P.stats()
    rec["stats"] = st
    rec["nnz_B"] = st["nnz"]
    rec["fill_ratio"] = st["nnz"] / Z
    rec["levels"] = list(P.levels())
    rec["update_values_ms"] = median([wall(P.update)[0] for _ in range(a.rounds)])
    note("update")
    for _ in range(2):
        P.ldiv(v, out=u)
    rec["ldiv_ms"] = median([wall(lambda: [P.ldiv(v, out=u) for _ in range(a.iters)])[0] / a.iters for _ in range(a.rounds)])
    x = P.solve(b)
    r = A.mul(x) - b
    rec["solve_residual"] = float(torch.linalg.norm(r) / torch.linalg.norm(b))
    note("ldiv and solve")
    cp, rv, nz = P.fill_matrix()
    P.close()
    Bm = esp.ExtendableSparseMatrix(esp.SparseMatrixCSC(N, N, cp, rv, nz))      # ILUAM's analysis + factorization of B, on a copy
    Bm.flush()
    Pw = esp.ILU0Preconditioner(Bm)
    Pw.close()
    ts = []
    for _ in range(a.rounds):
        t, Q = wall(lambda: esp.ILUAMPreconditioner(Bm))
        ts.append(t)
        Q.close()
    del Bm
    rec["create_iluam_of_B_ms"] = median(ts)
    rec["create_fill_ms"] = rec["create_ms"] - rec["ordering_ms"] - rec["create_iluam_of_B_ms"]
    out["lu"] = rec
    note("parts")
    # one solve to 1e-8: the direct solve (create + solve, what A.solve(b) does) against cg with ILU0 and ILUAM (create + cg)
    sol = {}
    sol["A.solve"] = {"ms": median([wall(lambda: A.solve(b))[0] for _ in range(a.rounds)]), "residual": rec["solve_residual"]}
    for name, make in (("cg+ilu0", esp.ILU0Preconditioner), ("cg+iluam", esp.ILUAMPreconditioner)):
        def run():
            Q = make(A)
            try:
                return esp.cg(A, b, Pl=Q, reltol=1e-8, maxiter=a.tol_maxiter, log=True)
            finally:
                Q.close()
        run()
        ts, log = [], None
        for _ in range(a.rounds):
            t, (_, log) = wall(run)
            ts.append(t)
        sol[name] = {"ms": median(ts), "iterations": log["iters"], "converged": log["isconverged"]}
    out["solve_1e-8"] = sol

    def rnd(x):
        if isinstance(x, float):
            return round(x, 4) if abs(x) >= 1e-3 else float("%.3e" % x)
        if isinstance(x, dict):
            return {k: rnd(y) for k, y in x.items()}
        return x
    print(json.dumps(rnd(out)))


def bench_lu_forms(a, torch, esp):
    """--kind lu --form panels | both: the forms of LUFactorization on fdrand n^3 side by side in alternating rounds in one process
    (both: the column form, the yardstick, takes part; panels: the panel form alone), CholeskyFactorization beside them: per round the
    create, a values-only update! and ldiv! on device vectors (--iters of them) of each.  Reported: every round's value, the median and
    the spread (max - min); whether each panel-form median lies below the column form's by more than the column form's spread; the
    ratio to Cholesky; the panel form's stats; |A x - b| / |b| for b = ones; and cg with ILU0 to 1e-8 (create + cg) from the same run."""
    import numpy as np
    A = esp.fdrand(a.n, a.n, a.n)
    d = A._d
    stream = torch.cuda.current_stream()
    d.ck(d.lib.esp_set_stream(d.h, C.c_void_p(stream.cuda_stream)))
    N, Z = A.n, A.nnz()
    v = torch.randn(N, dtype=torch.float64, device="cuda")
    u = torch.empty_like(v)
    b = torch.ones_like(v)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()                                   # (create, update!, ldiv! and the solvers return synchronised)
        return (time.perf_counter() - t0) * 1e3, r

    out = {"workload": "lu_forms_fdrand", "n": a.n, "N": N, "nnz": Z, "leaf_size": a.leaf_size, "rounds": a.rounds, "iters": a.iters,
           "form": a.form}
    Pw = esp.ILU0Preconditioner(A)     # builds the row-wise index the ordering shares, so that the creates below are their own
    Pw.close()
    P = esp.LUFactorization(A, a.leaf_size, form="panels")       # (a warm-up create: code objects, allocations)
    out["stats"], out["panel_stats"] = P.stats(), P.panel_stats()
    P.close()
    kinds = [("panels", lambda: esp.LUFactorization(A, a.leaf_size, form="panels")),
             ("cholesky", lambda: esp.CholeskyFactorization(A, a.leaf_size))]
    if a.form == "both":
        kinds.insert(0, ("columns", lambda: esp.LUFactorization(A, a.leaf_size)))
    rec = {name: {"create_ms": [], "update_values_ms": [], "ldiv_ms": []} for name, _ in kinds}
    resid = {}
    for r in range(a.rounds):
        for name, make in kinds:
            t, Q = wall(make)
            rec[name]["create_ms"].append(t)
            rec[name]["update_values_ms"].append(wall(Q.update)[0])
            Q.ldiv(v, out=u)
            rec[name]["ldiv_ms"].append(wall(lambda: [Q.ldiv(v, out=u) for _ in range(a.iters)])[0] / a.iters)
            if name not in resid:
                x = Q.solve(b)
                resid[name] = float(torch.linalg.norm(A.mul(x) - b) / torch.linalg.norm(b))
            Q.close()
            print("lu forms n=%d round %d %s: %s" % (a.n, r, name, json.dumps({k: x[-1] for k, x in rec[name].items()})), file=sys.stderr, flush=True)
    for name, _ in kinds:
        out[name] = {k: {"rounds": x, "median": float(np.median(x)), "spread": float(max(x) - min(x))} for k, x in rec[name].items()}
        out[name]["solve_residual"] = resid[name]
    keys = ("create_ms", "update_values_ms", "ldiv_ms")
    out["panels_over_cholesky"] = {k: out["panels"][k]["median"] / out["cholesky"][k]["median"] for k in keys}
    if a.form == "both":
        out["columns_over_panels"] = {k: out["columns"][k]["median"] / out["panels"][k]["median"] for k in keys}
        out["below_by_more_than_the_spread"] = {k: out["panels"][k]["median"] < out["columns"][k]["median"] - out["columns"][k]["spread"] for k in keys}

    def run():
        Q = esp.ILU0Preconditioner(A)
        try:
            return esp.cg(A, b, Pl=Q, reltol=1e-8, maxiter=a.tol_maxiter, log=True)
        finally:
            Q.close()
    run()
    ts, log = [], None
    for _ in range(a.rounds):
        t, (_, log) = wall(run)
        ts.append(t)
    out["solve_1e-8"] = {"cg+ilu0": {"ms": float(np.median(ts)), "rounds": ts, "iterations": log["iters"], "converged": log["isconverged"]}}

    def rnd(x):
        if isinstance(x, float):
            return round(x, 4) if abs(x) >= 1e-3 else float("%.3e" % x)
        if isinstance(x, dict):
            return {k: rnd(y) for k, y in x.items()}
        if isinstance(x, list):
            return [rnd(y) for y in x]
        return x
    print(json.dumps(rnd(out)))


def bench_cholesky(a, torch, esp):
    """CholeskyFactorization on fdrand n^3 beside LUFactorization, the yardstick, in the same process and the same alternating rounds
    (--lu-rounds R: LU takes part in the first R rounds only; 0: not at all): per round the ordering alone, the create, a values-only
    update! (the load and the numeric factorization) and ldiv! on device vectors of each.  Reported: every round's value, the median
    and the spread (max - min); symbolic_ms = create - ordering - update (the tables and the panels); the launch counts, nnz(L), the
    panel bytes, |A x - b| / |b| for b = ones; and one solve of A x = 1 to 1e-8 by cg with ILU0 (create + cg) from the same run."""
    import numpy as np
    A = esp.fdrand(a.n, a.n, a.n)
    d = A._d
    stream = torch.cuda.current_stream()
    d.ck(d.lib.esp_set_stream(d.h, C.c_void_p(stream.cuda_stream)))
    N, Z = A.n, A.nnz()
    v = torch.randn(N, dtype=torch.float64, device="cuda")
    u = torch.empty_like(v)
    b = torch.ones_like(v)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()                                   # (create, update!, ldiv! and the solvers return synchronised)
        return (time.perf_counter() - t0) * 1e3, r

    out = {"workload": "cholesky_fdrand", "n": a.n, "N": N, "nnz": Z, "leaf_size": a.leaf_size, "rounds": a.rounds, "lu_rounds": a.lu_rounds}
    Pw = esp.ILU0Preconditioner(A)     # builds the row-wise index the ordering shares, so that the creates below are their own
    Pw.close()
    P = esp.CholeskyFactorization(A, a.leaf_size)       # (a warm-up create: code objects, allocations)
    st = P.stats()
    P.close()
    kinds = [("cholesky", esp.CholeskyFactorization)]
    if a.lu_rounds > 0:
        kinds.append(("lu", esp.LUFactorization))
    rec = {name: {"create_ms": [], "update_values_ms": [], "ldiv_ms": []} for name, _ in kinds}
    ordering = []
    resid = {}
    for r in range(a.rounds):
        ordering.append(wall(lambda: esp.nested_dissection(A, a.leaf_size))[0])
        for name, cls in kinds:
            if name == "lu" and r >= a.lu_rounds:
                continue
            t, Q = wall(lambda: cls(A, a.leaf_size))
            rec[name]["create_ms"].append(t)
            rec[name]["update_values_ms"].append(wall(Q.update)[0])
            Q.ldiv(v, out=u)
            rec[name]["ldiv_ms"].append(wall(lambda: [Q.ldiv(v, out=u) for _ in range(a.iters)])[0] / a.iters)
            if name not in resid:
                x = Q.solve(b)
                resid[name] = float(torch.linalg.norm(A.mul(x) - b) / torch.linalg.norm(b))
            Q.close()
            print("cholesky n=%d round %d %s: %s" % (a.n, r, name, json.dumps({k: x[-1] for k, x in rec[name].items()})), file=sys.stderr, flush=True)
    out["ordering_ms"] = {"rounds": ordering, "median": float(np.median(ordering))}
    for name, _ in kinds:
        out[name] = {k: {"rounds": x, "median": float(np.median(x)), "spread": float(max(x) - min(x))} for k, x in rec[name].items()}
        out[name]["solve_residual"] = resid[name]
    c = out["cholesky"]
    c["symbolic_ms"] = c["create_ms"]["median"] - out["ordering_ms"]["median"] - c["update_values_ms"]["median"]
    c["stats"] = st
    c["panel_bytes"] = 8 * st["panel_doubles"]
    if "lu" in out:
        out["lu_over_cholesky"] = {k: out["lu"][k]["median"] / c[k]["median"] for k in ("create_ms", "update_values_ms", "ldiv_ms")}

    def run():
        Q = esp.ILU0Preconditioner(A)
        try:
            return esp.cg(A, b, Pl=Q, reltol=1e-8, maxiter=a.tol_maxiter, log=True)
        finally:
            Q.close()
    run()
    ts, log = [], None
    for _ in range(a.rounds):
        t, (_, log) = wall(run)
        ts.append(t)
    out["solve_1e-8"] = {"cg+ilu0": {"ms": float(np.median(ts)), "iterations": log["iters"], "converged": log["isconverged"]},
                         "cholesky create + solve": {"ms": c["create_ms"]["median"] + c["ldiv_ms"]["median"], "residual": resid["cholesky"]}}

    def rnd(x):
        if isinstance(x, float):
            return round(x, 4) if abs(x) >= 1e-3 else float("%.3e" % x)
        if isinstance(x, dict):
            return {k: rnd(y) for k, y in x.items()}
        if isinstance(x, list):
            return [rnd(y) for y in x]
        return x
    print(json.dumps(rnd(out)))


def bench_ilut(a, torch, esp):
    import numpy as np
    A = esp.fdrand(a.n, a.n, a.n)
    d = A._d
    stream = torch.cuda.current_stream()
    d.ck(d.lib.esp_set_stream(d.h, C.c_void_p(stream.cuda_stream)))
    N, Z = A.n, A.nnz()
    v = torch.randn(N, dtype=torch.float64, device="cuda")
    u = torch.empty_like(v)
    b = torch.ones_like(v)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()                                   # (create, update!, ldiv! and the solvers return synchronised)
        return (time.perf_counter() - t0) * 1e3, r

    def median(xs):
        return float(np.median(xs))

    par = dict(droptol=a.droptol, steps=a.steps, sweeps=a.sweeps)
    makes = {"ilu0": esp.ILU0Preconditioner, "iluam": esp.ILUAMPreconditioner, "iluk1": lambda M: esp.ILUKPreconditioner(M, 1),
             "ilut": lambda M: esp.ILUTPreconditioner(M, **par)}
    Pw = esp.ILU0Preconditioner(A)     # builds the row-wise index esp_mul shares, so that the creates below are their own
    Pw.close()
    creates = {k: [] for k in makes}
    for _ in range(a.rounds):          # alternated: one create of every kind per round
        for k, make in makes.items():
            t, P = wall(lambda: make(A))
            creates[k].append(t)
            P.close()
    out = {"workload": "ilut_fdrand", "n": a.n, "N": N, "nnz": Z, "rounds": a.rounds, **par}
    for k, make in makes.items():
        P = make(A)
        rec = {"create_ms": median(creates[k]), "create_min_max": [min(creates[k]), max(creates[k])]}
        rec["update_ms"] = median([wall(P.update)[0] for _ in range(a.rounds)])
        for _ in range(3):
            P.ldiv(v, out=u)
        rec["ldiv_ms"] = median([wall(lambda: [P.ldiv(v, out=u) for _ in range(a.iters)])[0] / a.iters for _ in range(a.rounds)])
        if hasattr(P, "levels"):
            rec["levels"] = list(P.levels())
        for name, fn in (("gmres", lambda: esp.gmres(A, b, Pl=P, restart=20, reltol=1e-8, maxiter=a.tol_maxiter, log=True)),
                         ("cg", lambda: esp.cg(A, b, Pl=P, reltol=1e-8, maxiter=a.tol_maxiter, log=True))):
            fn()
            ts, log = [], None
            for _ in range(a.rounds):
                t, (_, log) = wall(fn)
                ts.append(t)
            rec[name] = {"iterations": log["iters"], "converged": log["isconverged"], "ms": median(ts)}
        if k == "iluk1":
            rec["fill_ratio"] = P.stats()["nnz"] / Z
        if k == "ilut":
            st = P.stats()
            rec["stats"] = st
            rec["fill_ratio"] = st["nnz"] / Z
            rec["candidate_ratio"] = max([c for c, _ in st["steps"]] + [Z]) / Z
            # every array of the sweep once: rows, apos, old and new values, the row-wise index; A's values; per column pointers
            rec["sweep_bytes_min"] = st["nnz"] * (8 + 4 + 8 + 8 + 4 + 4) + Z * 8 + N * (8 + 4 + 8)
        P.close()
        out[k] = rec
    W1 = esp.ILUTPreconditioner(A, keep_pattern=True, **par)
    W5 = esp.ILUTPreconditioner(A, keep_pattern=True, **dict(par, sweeps=a.sweeps + 4))
    t1, t5 = [], []
    for _ in range(a.rounds):          # alternated as well
        t1.append(wall(W1.update)[0])
        t5.append(wall(W5.update)[0])
    out["ilut"]["warm_update_ms"] = median(t1)
    out["ilut"]["sweep_ms"] = (median(t5) - median(t1)) / 4
    out["ilut"]["sweep_nnz"] = W5.stats()["nnz"]
    W1.close()
    W5.close()

    def rnd(x):
        if isinstance(x, float):
            return round(x, 4)
        if isinstance(x, dict):
            return {k: rnd(y) for k, y in x.items()}
        if isinstance(x, list):
            return [rnd(y) for y in x]
        return x
    print(json.dumps(rnd(out)))


def bench_colored(a, torch, esp):
    import numpy as np
    A = esp.fdrand(a.n, a.n, a.n)
    d = A._d
    stream = torch.cuda.current_stream()
    d.ck(d.lib.esp_set_stream(d.h, C.c_void_p(stream.cuda_stream)))
    N, Z = A.n, A.nnz()
    v = torch.randn(N, dtype=torch.float64, device="cuda")
    u = torch.empty_like(v)
    b = torch.ones_like(v)
    inner = {"ilu0": esp.ILU0Preconditioner, "iluam": esp.ILUAMPreconditioner}[a.inner]

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()                                   # (create, update!, ldiv!, the colouring and cg return synchronised)
        return (time.perf_counter() - t0) * 1e3, r

    def median(xs):
        return float(np.median(xs))

    def measure(make):
        rec = {}
        ts = []
        for _ in range(a.rounds):
            t, P = wall(lambda: make(A))
            ts.append(t)
            P.close()
        rec["create_ms"] = median(ts)
        P = make(A)
        rec["update_values_ms"] = median([wall(P.update)[0] for _ in range(a.rounds)])
        for _ in range(3):
            P.ldiv(v, out=u)
        rec["ldiv_ms"] = median([wall(lambda: [P.ldiv(v, out=u) for _ in range(a.iters)])[0] / a.iters for _ in range(a.rounds)])
        if hasattr(P, "levels"):
            rec["levels"] = list(P.levels())
        fn = lambda: esp.cg(A, b, Pl=P, reltol=1e-8, maxiter=a.tol_maxiter, log=True)
        fn()
        ts, log = [], None
        for _ in range(a.rounds):
            t, (_, log) = wall(fn)
            ts.append(t)
        rec["cg"] = {"iterations": log["iters"], "converged": log["isconverged"], "ms": median(ts)}
        return rec, P

    out = {"workload": "colored_fdrand", "n": a.n, "N": N, "nnz": Z, "inner": a.inner, "rounds": a.rounds, "iters": a.iters}
    Pw = esp.ILU0Preconditioner(A)     # builds the row-wise index esp_mul shares, so that the creates below are their own
    Pw.close()
    for name, make in (("ilu0", esp.ILU0Preconditioner), ("iluam", esp.ILUAMPreconditioner),
                       ("colored_" + a.inner, lambda M: esp.ColoredPreconditioner(M, inner))):
        rec, P = measure(make)
        if name.startswith("colored"):
            rec["ncolors"] = P.ncolors
            rec["color_sizes"] = [len(c) for c in P.coloring()]
            nc = C.c_int64()
            rec["coloring_ms"] = median([wall(lambda: d.ck(d.lib.esp_graph_coloring(d.h, C.byref(nc), None, 0)))[0] for _ in range(a.rounds)])
            rec["coloring_rounds"] = nc.value
            rec["create_without_coloring_ms"] = rec["create_ms"] - rec["coloring_ms"]
        P.close()
        out[name] = rec
        print(json.dumps({name: rec}), file=sys.stderr, flush=True)   # (what is known so far, should a later phase be cut short)

    def rnd(x):
        if isinstance(x, float):
            return round(x, 4)
        if isinstance(x, dict):
            return {k: rnd(y) for k, y in x.items()}
        return x
    print(json.dumps(rnd(out)))


def bench_spai(a, torch, esp):
    """--kind spai0 | spai1 | spai1sym: set-up, values-only update!, ldiv! beside one mul! of A, and cg to 1e-8 beside Jacobi, ILU0 and
    ColoredPreconditioner (--inner) from the same run.  cg with the unsymmetrised spai1 is reported as it comes (M is not symmetric)."""
    import numpy as np
    A = esp.fdrand(a.n, a.n, a.n)
    d = A._d
    stream = torch.cuda.current_stream()
    d.ck(d.lib.esp_set_stream(d.h, C.c_void_p(stream.cuda_stream)))
    N, Z = A.n, A.nnz()
    v = torch.randn(N, dtype=torch.float64, device="cuda")
    u = torch.empty_like(v)
    b = torch.ones_like(v)
    inner = {"ilu0": esp.ILU0Preconditioner, "iluam": esp.ILUAMPreconditioner}[a.inner]

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()                                   # (create, update!, ldiv!, mul! and cg return synchronised)
        return (time.perf_counter() - t0) * 1e3, r

    def median(xs):
        return float(np.median(xs))

    def measure(make):
        rec = {}
        ts = []
        for _ in range(a.rounds):
            t, P = wall(lambda: make(A))
            ts.append(t)
            P.close()
        rec["setup_ms"] = median(ts)
        P = make(A)
        rec["update_ms"] = median([wall(P.update)[0] for _ in range(a.rounds)])
        for _ in range(3):
            P.ldiv(v, out=u)
        rec["ldiv_ms"] = median([wall(lambda: [P.ldiv(v, out=u) for _ in range(a.iters)])[0] / a.iters for _ in range(a.rounds)])
        fn = lambda: esp.cg(A, b, Pl=P, reltol=1e-8, maxiter=a.tol_maxiter, log=True)
        fn()
        ts, log = [], None
        for _ in range(a.rounds):
            t, (_, log) = wall(fn)
            ts.append(t)
        rec["cg"] = {"iterations": log["iters"], "converged": log["isconverged"], "ms": median(ts)}
        return rec, P

    out = {"workload": "spai_fdrand", "kind": a.kind, "n": a.n, "N": N, "nnz": Z, "rounds": a.rounds, "iters": a.iters}
    for _ in range(3):
        A.mul(v, out=u)                            # (builds the row-wise index mul! and the creates below share)
    out["mul_ms"] = median([wall(lambda: [A.mul(v, out=u) for _ in range(a.iters)])[0] / a.iters for _ in range(a.rounds)])
    spai = {"spai0": lambda M: esp.SPAIPreconditioner(M, 0), "spai1": lambda M: esp.SPAIPreconditioner(M, 1),
            "spai1sym": lambda M: esp.SPAIPreconditioner(M, 1, True)}[a.kind]
    for name, make in (("jacobi", esp.JacobiPreconditioner), ("ilu0", esp.ILU0Preconditioner),
                       ("colored_" + a.inner, lambda M: esp.ColoredPreconditioner(M, inner)), (a.kind, spai)):
        rec, P = measure(make)
        if name == a.kind:
            rec["stats"] = P.stats()
        P.close()
        out[name] = rec
        print(json.dumps({name: rec}), file=sys.stderr, flush=True)   # (what is known so far, should a later phase be cut short)

    def rnd(x):
        if isinstance(x, float):
            return round(x, 4)
        if isinstance(x, dict):
            return {k: rnd(y) for k, y in x.items()}
        return x
    print(json.dumps(rnd(out)))


def bench_many(a, torch, esp):
    """--nrhs K[,K...] with --kind cholesky | lu [--form columns|panels] | mul: several right-hand sides in one call
    (esp_precon_ldiv_many / esp_mul_many) against K single-vector calls of the same build in the same process, on fdrand n^3 and device
    arrays.  --rounds alternating rounds; a round times --iters repetitions of the one call, then of the K calls, and reports the mean
    of each.  Per K: every round's value, the medians, the spread (max - min), the time per column and the ratio K singles / one call."""
    import numpy as np
    A = esp.fdrand(a.n, a.n, a.n)
    d = A._d
    d.ck(d.lib.esp_set_stream(d.h, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    N = A.n
    ks = [int(x) for x in str(a.nrhs).split(",")]
    out = {"workload": "many_rhs_fdrand", "kind": a.kind, "form": a.form if a.kind == "lu" else None, "n": a.n, "N": N, "nnz": A.nnz(),
           "leaf_size": a.leaf_size, "rounds": a.rounds, "iters": a.iters, "nrhs": {}}
    if a.kind == "mul":
        P, rows = None, A.m
        one, many = (lambda x, r: A.mul(x, r)), (lambda X, R: A.mul(X, R))
    else:
        t0 = time.perf_counter()
        if a.kind == "iluam":
            P = esp.ILUAMPreconditioner(A)
        elif a.kind == "colored":
            P = esp.ColoredPreconditioner(A, esp.ILUAMPreconditioner)
        else:
            P = esp.CholeskyFactorization(A, a.leaf_size) if a.kind == "cholesky" else esp.LUFactorization(A, a.leaf_size, form=a.form)
        out["create_ms"] = (time.perf_counter() - t0) * 1e3
        out["stats"] = P.launches() if a.kind in ("iluam", "colored") else P.stats()
        rows = N
        one, many = (lambda x, r: P.ldiv(x, r)), (lambda X, R: P.ldiv(X, R))

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            fn()                                   # (every call returns synchronised)
        return (time.perf_counter() - t0) * 1e3 / a.iters

    for k in ks:
        X = torch.randn((k, N), dtype=torch.float64, device="cuda").t()
        R = torch.empty((k, rows), dtype=torch.float64, device="cuda").t()
        cols = [(X[:, r], torch.empty(rows, dtype=torch.float64, device="cuda")) for r in range(k)]
        singles = lambda: [one(x, r) for x, r in cols]
        for _ in range(max(a.warmup, 1)):
            many(X, R), singles()
        assert all(bool((R[:, r].view(torch.int64) == cols[r][1].view(torch.int64)).all()) for r in range(k)), "the columns differ"
        rec = {"many_ms": [], "singles_ms": []}
        for _ in range(a.rounds):
            rec["many_ms"].append(wall(lambda: many(X, R)))
            rec["singles_ms"].append(wall(singles))
        res = {}
        for name, v in rec.items():
            res[name] = {"rounds": [round(x, 4) for x in v], "median": round(float(np.median(v)), 4), "spread": round(max(v) - min(v), 4)}
        res["many_ms_per_column"] = round(res["many_ms"]["median"] / k, 4)
        res["singles_ms_per_column"] = round(res["singles_ms"]["median"] / k, 4)
        res["ratio_singles_over_many"] = round(res["singles_ms"]["median"] / res["many_ms"]["median"], 3)
        if hasattr(P, "many_stats"):               # (a build from before esp_precon_many_stats has none: the column loop)
            res["many_stats"] = P.many_stats()
        out["nrhs"][str(k)] = res
    if P is not None:
        P.close()
    print(json.dumps(out))


def bench_cg_many(a, torch, esp):
    """--nrhs K[,K...] with --kind cg: cg(A, B) with K columns in one call (esp_cg_many) against K single cg calls of the same build in
    the same process, in the shape of bench_many: --rounds alternating rounds of one solve each (default tolerance, at most --iters
    iterations), after an assertion that the columns of the two agree bit for bit"""
    import numpy as np
    A = esp.fdrand(a.n, a.n, a.n)
    d = A._d
    d.ck(d.lib.esp_set_stream(d.h, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    N = A.n
    name = a.cg_only or "ilu0"
    P = {"identity": lambda A: None, "jacobi": esp.JacobiPreconditioner, "ilu0": esp.ILU0Preconditioner,
         "iluam": esp.ILUAMPreconditioner}[name](A)
    ks = [int(x) for x in str(a.nrhs).split(",")]
    out = {"workload": "cg_many_fdrand", "kind": name, "n": a.n, "N": N, "nnz": A.nnz(), "rounds": a.rounds, "maxiter": a.iters, "nrhs": {}}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()                                       # (every call returns synchronised)
        return (time.perf_counter() - t0) * 1e3

    torch.manual_seed(1)
    for k in ks:
        B = torch.randn((k, N), dtype=torch.float64, device="cuda").t()
        X = torch.empty((k, N), dtype=torch.float64, device="cuda").t()
        xs = [torch.empty(N, dtype=torch.float64, device="cuda") for _ in range(k)]
        bs = [B[:, r].contiguous() for r in range(k)]

        def many(log=False):
            X.zero_()
            return esp.cg(A, B, Pl=P, x=X, maxiter=a.iters, log=log)

        def singles(log=False):
            for x in xs:
                x.zero_()
            return [esp.cg(A, b, Pl=P, x=x, maxiter=a.iters, log=log) for b, x in zip(bs, xs)]

        for _ in range(max(min(a.warmup, 2), 1)):
            many(), singles()
        got = many(log=True)
        want = singles(log=True)
        logs = got[1]                              # (a 2-D B of one column takes the many-column entry as well: a list of one dict)
        for r in range(k):
            col = X[:, r]
            assert bool((col.contiguous().view(torch.int64) == want[r][0].view(torch.int64)).all()), "x differs in column %d" % r
            assert logs[r]["iters"] == want[r][1]["iters"] and logs[r]["isconverged"] == want[r][1]["isconverged"], "column %d" % r
            assert np.array_equal(np.concatenate([[logs[r]["r0"]], logs[r]["resnorm"]]).view(np.uint64),
                                  np.concatenate([[want[r][1]["r0"]], want[r][1]["resnorm"]]).view(np.uint64)), "history of column %d" % r
        rec = {"many_ms": [], "singles_ms": []}
        for _ in range(a.rounds):
            rec["many_ms"].append(wall(many))
            rec["singles_ms"].append(wall(singles))
        res = {"iterations": [int(l["iters"]) for l in logs]}
        for what, v in rec.items():
            res[what] = {"rounds": [round(x, 3) for x in v], "median": round(float(np.median(v)), 3), "spread": round(max(v) - min(v), 3)}
        res["many_ms_per_column"] = round(res["many_ms"]["median"] / k, 3)
        res["singles_ms_per_column"] = round(res["singles_ms"]["median"] / k, 3)
        res["ratio_singles_over_many"] = round(res["singles_ms"]["median"] / res["many_ms"]["median"], 3)
        out["nrhs"][str(k)] = res
    if P is not None:
        P.close()
    print(json.dumps(out))


def bench_gmres_many(a, torch, esp):
    """--nrhs K[,K...] with --kind gmres: gmres(A, B) with K columns in one call (esp_gmres_many) against K single gmres calls of the
    same build in the same process, in the shape of bench_cg_many: --rounds alternating rounds of one solve each (reltol = 0 and
    --iters iterations, so every column takes all of them), after an assertion that the columns of the two agree bit for bit"""
    import numpy as np
    A = esp.fdrand(a.n, a.n, a.n)
    d = A._d
    d.ck(d.lib.esp_set_stream(d.h, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    N = A.n
    name = a.cg_only or "ilu0"
    P = {"identity": lambda A: None, "jacobi": esp.JacobiPreconditioner, "ilu0": esp.ILU0Preconditioner,
         "iluam": esp.ILUAMPreconditioner}[name](A)
    ks = [int(x) for x in str(a.nrhs).split(",")]
    kw = dict(restart=a.restart, orth_meth=a.orth, maxiter=a.iters, reltol=0.0)
    out = {"workload": "gmres_many_fdrand", "kind": name, "n": a.n, "N": N, "nnz": A.nnz(), "rounds": a.rounds, "maxiter": a.iters,
           "restart": a.restart, "orth": a.orth, "nrhs": {}}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()                                       # (every call returns synchronised)
        return (time.perf_counter() - t0) * 1e3

    def history(log):
        return np.concatenate([[log["r0"]], log["resnorm"]]).view(np.uint64)

    torch.manual_seed(1)
    for k in ks:
        B = torch.randn((k, N), dtype=torch.float64, device="cuda").t()
        X = torch.empty((k, N), dtype=torch.float64, device="cuda").t()
        xs = [torch.empty(N, dtype=torch.float64, device="cuda") for _ in range(k)]
        bs = [B[:, r].contiguous() for r in range(k)]

        def many(log=False):
            X.zero_()
            return esp.gmres(A, B, Pl=P, x=X, log=log, **kw)

        def singles(log=False):
            for x in xs:
                x.zero_()
            return [esp.gmres(A, b, Pl=P, x=x, log=log, **kw) for b, x in zip(bs, xs)]

        for _ in range(max(min(a.warmup, 2), 1)):
            many(), singles()
        logs = many(log=True)[1]                   # (a 2-D B of one column takes the many-column entry as well: a list of one dict)
        want = singles(log=True)
        for r in range(k):
            assert bool((X[:, r].contiguous().view(torch.int64) == want[r][0].view(torch.int64)).all()), "x differs in column %d" % r
            assert all(logs[r][key] == want[r][1][key] for key in ("iters", "mvps", "reorth", "isconverged")), "column %d" % r
            assert np.array_equal(history(logs[r]), history(want[r][1])), "history of column %d" % r
        rec = {"many_ms": [], "singles_ms": []}
        for _ in range(a.rounds):
            rec["many_ms"].append(wall(many))
            rec["singles_ms"].append(wall(singles))
        res = {"iterations": [int(l["iters"]) for l in logs], "reorth": [int(l["reorth"]) for l in logs]}
        for what, v in rec.items():
            res[what] = {"rounds": [round(x, 3) for x in v], "median": round(float(np.median(v)), 3), "spread": round(max(v) - min(v), 3)}
        res["many_ms_per_column"] = round(res["many_ms"]["median"] / k, 3)
        res["singles_ms_per_column"] = round(res["singles_ms"]["median"] / k, 3)
        res["ratio_singles_over_many"] = round(res["singles_ms"]["median"] / res["many_ms"]["median"], 3)
        out["nrhs"][str(k)] = res
    if P is not None:
        P.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kind", choices=["point", "iluam", "cg", "bicgstabl", "gmres", "gmres-trace", "block", "block-trace", "block-trace-diff", "amg", "iluk", "colored", "spai0", "spai1", "spai1sym", "ilut", "lu", "cholesky", "mul"], default="point")
    ap.add_argument("--nrhs", default="", help="--kind cholesky | lu | mul | cg: K or K,K,...: K right-hand sides in one call against K single calls")
    ap.add_argument("--leaf-size", type=int, default=32)
    ap.add_argument("--form", choices=["columns", "panels", "both"], default="columns",
                    help="--kind lu: columns: the column form's breakdown; panels / both: the forms side by side in alternating rounds")
    ap.add_argument("--lu-rounds", type=int, default=0, help="--kind cholesky: the rounds LUFactorization, the yardstick, takes part in")
    ap.add_argument("--droptol", type=float, default=1e-3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--sweeps", type=int, default=3)
    ap.add_argument("--inner", choices=["ilu0", "iluam"], default="iluam")
    ap.add_argument("--k", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--block-config", choices=["a", "b", "c", "d", "e"], default="b")
    ap.add_argument("--dirs", nargs=2, default=None)
    ap.add_argument("--cg-only", choices=["identity", "jacobi", "ilu0", "iluam"], default=None)
    ap.add_argument("--tol-n", type=int, default=0)
    ap.add_argument("--tol-maxiter", type=int, default=100000)
    ap.add_argument("--cpu-model", action="store_true")
    ap.add_argument("--ls", default="1,2,4")
    ap.add_argument("--orths", default="mgs,dgks")
    ap.add_argument("--restart", type=int, default=20, help="--kind gmres --nrhs: the length of a cycle")
    ap.add_argument("--orth", choices=["mgs", "cgs", "dgks"], default="mgs", help="--kind gmres --nrhs: the orthogonalisation")
    ap.add_argument("--no-composed", action="store_true")
    ap.add_argument("--coarsen", choices=["sa", "rs"], default="sa")
    ap.add_argument("--cd-n", type=int, default=64)
    ap.add_argument("--cd-pe", type=float, default=4.0)
    a = ap.parse_args()
    if a.kind == "block-trace-diff":
        return block_trace_diff(a)
    import torch
    torch.cuda.init()
    from esparse_loader import load
    esp = load()
    if a.nrhs and a.kind == "cg":
        return bench_cg_many(a, torch, esp)
    if a.nrhs and a.kind == "gmres":
        return bench_gmres_many(a, torch, esp)
    if a.nrhs or a.kind == "mul":
        if a.kind not in ("cholesky", "lu", "mul", "iluam", "colored") or not a.nrhs or (a.kind == "lu" and a.form == "both"):
            ap.error("--nrhs K goes with --kind cholesky, --kind lu --form columns|panels, --kind iluam, --kind colored, --kind mul, --kind cg "
                     "or --kind gmres")
        return bench_many(a, torch, esp)
    if a.kind == "iluam":
        return bench_iluam(a, torch, esp)
    if a.kind == "cg":
        return bench_cg(a, torch, esp)
    if a.kind == "bicgstabl":
        return bench_bicgstabl(a, torch, esp)
    if a.kind == "gmres":
        return bench_gmres(a, torch, esp)
    if a.kind == "gmres-trace":
        return bench_gmres_trace(a, torch, esp)
    if a.kind == "block":
        return bench_block(a, torch, esp)
    if a.kind == "block-trace":
        return bench_block_trace(a, torch, esp)
    if a.kind == "iluk":
        return bench_iluk(a, torch, esp)
    if a.kind == "ilut":
        return bench_ilut(a, torch, esp)
    if a.kind == "lu":
        return bench_lu(a, torch, esp) if a.form == "columns" else bench_lu_forms(a, torch, esp)
    if a.kind == "cholesky":
        return bench_cholesky(a, torch, esp)
    if a.kind == "amg":
        return bench_amg(a, torch, esp)
    if a.kind == "colored":
        return bench_colored(a, torch, esp)
    if a.kind in ("spai0", "spai1", "spai1sym"):
        return bench_spai(a, torch, esp)
    A = esp.fdrand(a.n, a.n, a.n)
    d = A._d
    stream = torch.cuda.current_stream()
    d.ck(d.lib.esp_set_stream(d.h, C.c_void_p(stream.cuda_stream)))
    N = A.n
    Z = A.nnz()
    v = torch.randn(N, dtype=torch.float64, device="cuda")
    u = torch.empty_like(v)
    b = torch.ones_like(v)

    def timed(fn, reps):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    out = {"workload": "precon_fdrand", "n": a.n, "N": N, "nnz": Z}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    Pi = esp.ILU0Preconditioner(A)           # first build: split layout + xdiag + scaled values (row-wise index included)
    e1.record()
    e1.synchronize()
    out["ilu0_create_first_ms"] = e0.elapsed_time(e1)
    e0.record()
    Pi2 = esp.ILU0Preconditioner(A)          # a create with the row-wise index already built
    e1.record()
    e1.synchronize()
    out["ilu0_create_ms"] = e0.elapsed_time(e1)
    Pi2.close()
    Pj = esp.JacobiPreconditioner(A)
    out["jacobi_ldiv_ms"] = timed(lambda: Pj.ldiv(v, out=u), a.iters)
    out["ilu0_ldiv_ms"] = timed(lambda: Pi.ldiv(v, out=u), a.iters)
    out["ilu0_update_values_ms"] = timed(lambda: Pi.update(), max(10, a.iters // 5))
    out["jacobi_update_values_ms"] = timed(lambda: Pj.update(), max(10, a.iters // 5))

    def run_simple(k):
        x = torch.zeros_like(v)
        esp.simple(A, b, u=x, Pl=Pi, maxiter=k, reltol=0.0)

    t_long = timed(lambda: run_simple(a.iters + 1), 3)
    t_short = timed(lambda: run_simple(1), 3)
    out["simple_ilu0_step_ms"] = (t_long - t_short) / a.iters
    t_long = timed(lambda: esp.simple(A, b, u=torch.zeros_like(v), Pl=Pj, maxiter=a.iters + 1, reltol=0.0), 3)
    t_short = timed(lambda: esp.simple(A, b, u=torch.zeros_like(v), Pl=Pj, maxiter=1, reltol=0.0), 3)
    out["simple_jacobi_step_ms"] = (t_long - t_short) / a.iters
    zp = (Z - N) // 2   # entries of each part (symmetric pattern)
    gb = {
        "ilu0_ldiv": (2 * 4 * (N + 1) + 12 * 2 * zp + 16 * N + 8 * N + 8 * N + 8 * N) / 1e9,
        "jacobi_ldiv": 24 * N / 1e9,
        "residual": (12 * Z + 32 * N) / 1e9,
    }
    gb["simple_ilu0_step"] = gb["ilu0_ldiv"] + 8 * N / 1e9 + gb["residual"]   # (+ u read by the fused u .-= upd)
    out["algorithmic_GB"] = {k: round(x, 3) for k, x in gb.items()}
    out["GBps"] = {"ilu0_ldiv": round(gb["ilu0_ldiv"] / out["ilu0_ldiv_ms"] * 1e3, 1),
                   "jacobi_ldiv": round(gb["jacobi_ldiv"] / out["jacobi_ldiv_ms"] * 1e3, 1),
                   "simple_ilu0_step": round(gb["simple_ilu0_step"] / out["simple_ilu0_step_ms"] * 1e3, 1)}
    Pi.close()
    Pj.close()
    print(json.dumps({k: (round(x, 4) if isinstance(x, float) else x) for k, x in out.items()}))


if __name__ == "__main__":
    main()
