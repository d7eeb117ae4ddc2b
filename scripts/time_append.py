"""Timing of ``Observations.append`` against conditioning from scratch (MI355X).

For fp64 and fp32, n = 16384 observations (D = 8, EQ kernel, noise 0.1) and q new points, q in {1, 8, 16, 128, 1024}:

  append    ``obs.append(f(x_new, noise), y_new)`` + ``post(xs).marginals()`` at N* = 2048 test points, the factor growing IN PLACE in
            its capacity buffer (every repetition starts from the same factor of order n: the buffer's fill count is rewound, which
            only this script does);
  scratch   a fresh ``Observations`` on the n + q points doing the same (kernel matrix, factorisation, solves).

Repetitions of the two are interleaved and the medians reported (HIP events around each; one warm-up round).  The append is then
run once more with its phases timed one by one (events around each, so the phases do not overlap as they may in the total): the
cross-covariance build ``k(x, x_new)`` and ``k(x_new)``, the solve ``V = L11^{-1} K12``, the border launches (``gpk_potrf_border``),
the copy of the factor into a new capacity buffer (paid by the first append and after growth only), and the prediction.  The last
line per dtype is the crossover: the smallest q / n of the table at which conditioning from scratch is faster.

    python scripts/time_append.py [n] [reps]
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import stheno_amd.torch as st  # noqa: E402
from stheno_amd import B, matrix, ops  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
QS = (1, 8, 16, 128, 1024)
NS, D = 2048, 8
dev = torch.device("cuda")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def main():
    results = []
    for dtype in (torch.float64, torch.float32):
        B.epsilon = 1e-12 if dtype == torch.float64 else 1e-6
        g = torch.Generator().manual_seed(0)
        x = torch.randn(N + 1 + max(QS), D, generator=g, dtype=torch.float64).to(dev, dtype)
        y = (torch.sin(x.sum(-1, keepdim=True)) + 0.1 * torch.randn(N + 1 + max(QS), 1, generator=g, dtype=torch.float64).to(dev, dtype))
        xs = torch.randn(NS, D, generator=g, dtype=torch.float64).to(dev, dtype)
        f = st.GP(st.EQ().stretch(2.0))
        measure = f.measure

        def predict(obs):
            return (measure | obs)(f)(xs).marginals()

        base = st.Obs(f(x[:N], 0.1), y[:N])
        predict(base)
        chol0 = base._K_x[measure]._chol
        # one append of one point: the factor moves into its capacity buffer (the copy is timed below)
        first, t_first = timed(lambda: base.append(f(x[N : N + 1], 0.1), y[N : N + 1]))
        grow = first._K_x[measure]._chol._grow
        n1 = N + 1
        crossover = None
        for q in QS:
            xn, yn = x[n1 : n1 + q], y[n1 : n1 + q]
            if n1 + q > grow.buf.shape[0]:
                print(f"# q = {q}: does not fit the capacity buffer of order {grow.buf.shape[0]}; skipped")
                continue

            def append():
                grow.filled = n1
                new = first.append(f(xn, 0.1), yn)
                return predict(new)

            def scratch():
                return predict(st.Obs(f(x[: n1 + q], 0.1), y[: n1 + q]))

            append(), scratch()
            ta, ts = [], []
            for _ in range(REPS):
                (ma, va), t = timed(append)
                ta.append(t)
                (ms_, vs_), t = timed(scratch)
                ts.append(t)
            err_mean = float((ma - ms_).abs().max() / ms_.abs().max())
            err_var = float((va - vs_).abs().max() / vs_.abs().max())
            # the phases of one append, one by one
            kernel = measure.kernels[f]
            chol = first._K_x[measure]._chol
            (k12, k22), t_build = timed(lambda: (kernel.pairwise(x[:n1], xn), kernel.pairwise(xn, None, lower=True, diag_add=B.epsilon,
                                                                                            diag_vec=torch.full((q,), 0.1, dtype=dtype, device=dev))))
            phases = {"solve": 0.0, "border": 0.0}
            be = ops.get_backend()
            solve0, border0 = matrix.Chol.solve, be.potrf_border

            def solve(self, b):
                out, t = timed(lambda: solve0(self, b))
                phases["solve"] += t
                return out

            def border(*a, **k):
                out, t = timed(lambda: border0(*a, **k))
                phases["border"] += t
                return out

            matrix.Chol.solve, be.potrf_border = solve, border
            try:
                grow.filled = n1
                grown, t_append = timed(lambda: chol.append(k12, k22))
            finally:
                matrix.Chol.solve = solve0
                del be.potrf_border
            _, t_copy = timed(lambda: be.copy(chol.l, out=torch.empty_like(grow.buf)[:n1, :n1]))
            grow.filled = n1
            new = first.append(f(xn, 0.1), yn)
            _, t_predict = timed(lambda: predict(new))
            row = dict(dtype=str(dtype)[6:], n=n1, q=q, append_ms=statistics.median(ta), scratch_ms=statistics.median(ts),
                       build_ms=t_build, solve_ms=phases["solve"], border_ms=phases["border"], copy_ms=t_copy, predict_ms=t_predict,
                       rel_mean=err_mean, rel_var=err_var)
            results.append(row)
            print("{dtype} n={n} q={q:5d}  append {append_ms:8.3f} ms  scratch {scratch_ms:8.3f} ms  | build {build_ms:7.3f}  solve {solve_ms:8.3f}  "
                  "border {border_ms:7.3f}  (buffer copy {copy_ms:7.3f})  predict {predict_ms:7.3f} | rel. diff mean {rel_mean:.1e} var {rel_var:.1e}".format(**row),
                  flush=True)
            if crossover is None and row["scratch_ms"] < row["append_ms"]:
                crossover = q / n1
            grow.filled = n1
        print(f"{str(dtype)[6:]}: first append (with the copy into the buffer) {t_first:.3f} ms; crossover q / n: "
              f"{'none up to q = %d (%.3f)' % (QS[-1], QS[-1] / n1) if crossover is None else '%.4f' % crossover}", flush=True)
        del base, first, grow, chol0
        torch.cuda.empty_cache()
    print(json.dumps(results))


if __name__ == "__main__":
    main()
