"""Times the point preconditioners and simple! on the device CSC of fdrand(n,n,n) (default 256^3): Jacobi and ILU0 ldiv!
on device vectors, update! values-only, the first build after a pattern change (create), and one simple! step with ILU0
(averaged over --iters steps).  The library runs on torch's current stream (esp_set_stream), so device events bracket its
work; every call also returns synchronised.  Prints one JSON line: ms and the algorithmic bytes of DESIGN.md.

    python tools/precon_bench.py [--n 256] [--iters 50] [--warmup 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    from esparse_loader import load
    esp = load()
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
