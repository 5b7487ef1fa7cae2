"""Times transpose, transpose(A)*x, issymmetric, opnorm and norm on the device CSC (esp_transpose, esp_mul_transpose,
esp_issymmetric, esp_opnorm, esp_norm) on fdrand(n,n,n) (default 256^3).  Every call returns synchronised, so host wall-clock
brackets one call; a transpose allocates its result (a new matrix), which is freed and the device synchronised BEFORE the next
timed call, so no free lands inside the window.  transpose(A)*x runs on CUDA torch tensors (device pointers, as esp_mul's
consumers do); opnorm(A, Inf) is timed with the row-wise index current (the warm-up builds it).  Prints one JSON line: ms per
call (mean and min), the algorithmic bytes of DESIGN.md §5d and the fraction of 8 TB/s they reach.  --only NAME times one
case (a kernel profile of one operation: rocprofv3 --kernel-trace --stats).

    python tools/linalg_bench.py [--n 256] [--iters 5] [--warmup 1]
        [--only transpose|transpose_generic|mul_transpose|issymmetric|opnorm1|opnorminf|norm2]
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
    ap.add_argument("--only", default=None, help="time this case only")
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    from esparse_loader import load
    esp = load()
    A = esp.fdrand(a.n, a.n, a.n, seed=0x5EED0002)
    m, n, Z = A.m, A.n, A.nnz()
    want = (lambda name: a.only is None or a.only == name)
    x = torch.rand(m, dtype=torch.float64, device="cuda")
    r = torch.empty(n, dtype=torch.float64, device="cuda")

    def timed(fn):
        ts, res = [], None
        for k in range(a.warmup + a.iters):
            res = None                                    # the previous result is freed outside the window
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()                                    # (returns synchronised)
            if k >= a.warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.mean(ts)), float(np.min(ts))

    # algorithmic bytes
    cases = [
        ("transpose", lambda: A.transpose(), 32 * Z + 8 * (m + 1) + 8 * (n + 1)),
        ("transpose_generic", lambda: A.transpose(path=1), 32 * Z + 8 * (m + 1) + 8 * (n + 1)),
        ("mul_transpose", lambda: A.mul_transpose(x, out=r), 16 * Z + 8 * (n + 1) + 8 * m + 8 * n),
        ("issymmetric", lambda: A.issymmetric(), 16 * Z + 8 * (n + 1)),
        ("opnorm1", lambda: A.opnorm(1), 8 * Z + 8 * (n + 1)),
        ("opnorminf", lambda: A.opnorm(float("inf")), 8 * Z + 8 * (m + 1)),
        ("norm2", lambda: A.norm(2), 16 * Z),  # two passes over nzval (max |v|, then the scaled squares)
    ]
    out = {"workload": "linalg_fdrand", "n": a.n, "N": n, "nnz": Z}
    for name, fn, nbytes in cases:
        if not want(name):
            continue
        ms, mn = timed(fn)
        g = nbytes / 1e9
        out[name] = {"ms": round(ms, 3), "ms_min": round(mn, 3), "algorithmic_GB": round(g, 3),
                     "frac_8TBps": round(g / (ms * 1e-3) / (PEAK / 1e9), 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
