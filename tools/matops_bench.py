"""Times the device matrix algebra (esp_matmul, esp_add, esp_diag_scale) on fdrand(n,n,n) (default 256^3): A*A automatic and
with each tier forced (esp_debug_matmul_tier), A+B with B on A's pattern (another fdrand) and with a shifted pattern (A*S, S the
shift by one column), and D*A.  Every call returns synchronised and allocates its result (a new matrix), so host wall-clock
brackets one call: the result handle, its device allocations and the host reads of nnz included.  The previous result is freed
and the device synchronised BEFORE each timed call, so no free lands inside the window.  Prints one JSON line: ms per call
(mean and min), the algorithmic bytes of DESIGN.md §5c (16 (nnz A + nnz B + nnz C) + 8 (A.n + B.n + C.n + 3)) and the
fraction of 8 TB/s they reach.  --only NAME times one case (a kernel profile of one operation: rocprofv3 --kernel-trace --stats).

    python tools/matops_bench.py [--n 256] [--iters 5] [--warmup 1] [--skip-generic] [--only AxA|AxA_fused|AxA_generic|ApB_same_pattern|ApB_shifted|DxA]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--skip-generic", action="store_true", help="leave out A*A with every column in the generic tier")
    ap.add_argument("--only", default=None, help="time this case only")
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    from esparse_loader import load
    esp = load()
    A = esp.fdrand(a.n, a.n, a.n, seed=0x5EED0002)
    B = esp.fdrand(a.n, a.n, a.n, seed=0x5EED0003)   # same pattern, other values
    N = A.n
    want = (lambda name: a.only is None or a.only == name)
    Bs = None
    if want("ApB_shifted"):
        S = esp.ExtendableSparseMatrix.from_coo(np.arange(1, N, dtype=np.int64), np.arange(2, N + 1, dtype=np.int64), np.ones(N - 1), N, N)
        Bs = A * S                                        # A's pattern shifted by one column
        del S
    d = torch.rand(N, dtype=torch.float64, device="cuda") + 0.5
    D = esp.Diagonal(d)

    def timed(fn):
        ts, r = [], None
        for k in range(a.warmup + a.iters):
            r = None                                      # the previous result is freed outside the window
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()                                      # (returns synchronised)
            if k >= a.warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.mean(ts)), float(np.min(ts)), r

    def gb(nnz_a, nnz_b, nnz_c, na, nb, nc):
        return (16 * (nnz_a + nnz_b + nnz_c) + 8 * (na + nb + nc + 3)) / 1e9

    out = {"workload": "matops_fdrand", "n": a.n, "N": N, "nnz": A.nnz()}
    rows = {}
    cases = [("AxA", lambda: A.matmul(A)), ("AxA_fused", lambda: A.matmul(A, tier=1))]
    if not a.skip_generic:
        cases.append(("AxA_generic", lambda: A.matmul(A, tier=2)))
    for name, fn in cases:
        if want(name):
            ms, mn, C = timed(fn)
            rows[name] = (ms, mn, gb(A.nnz(), A.nnz(), C.nnz(), N, N, N), C.nnz())
            del C
    for name, X in (("ApB_same_pattern", B), ("ApB_shifted", Bs)):
        if want(name):
            ms, mn, C = timed(lambda: A + X)
            rows[name] = (ms, mn, gb(A.nnz(), X.nnz(), C.nnz(), N, N, N), C.nnz())
            del C
    if want("DxA"):
        ms, mn, C = timed(lambda: D * A)
        rows["DxA"] = (ms, mn, (16 * 2 * A.nnz() + 8 * (2 * (N + 1) + N)) / 1e9, C.nnz())
        del C
    for name, (ms, mn, g, z) in rows.items():
        out[name] = {"ms": round(ms, 3), "ms_min": round(mn, 3), "algorithmic_GB": round(g, 3), "nnz_C": z, "frac_8TBps": round(g / (ms * 1e-3) / (PEAK / 1e9), 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
