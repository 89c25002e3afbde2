"""Where the bounds of tests/test_elementwise_kernels_gpu.py come from.  CPU only:

    python tests/diagnostics/elementwise_bounds.py [inject] [colsum] [linear] [caption]

Each part runs the fp32 restatements of tests/_elementwise_ref.py (numpy, one rounding per operation, the kernel's
summation grouping) on the very inputs the test builds and measures them against fp64.  For the sums the figure is
the largest |fp32 sum - fp64 sum| in fp32 ulps of sum |terms|, per case and worst per family; the test allows 4x each
family's worst (SUM_UNITS: another legal fp32 summation order).  For the caption pooling it is the largest
difference in fp16 ulps between the restatement and fp64 through the same fp16 rounding points, with numpy's expf
and with expf moved by one fp32 ulp either way (CAPTION_ULPS: 4x).  Each restatement is also checked against the
test's own fp64 tolerance (E.check64), i.e. it is self-consistent with a plain fp64 sum to the printed figure.
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import _elementwise_ref as E  # noqa: E402
import test_elementwise_kernels_gpu as T  # noqa: E402

f64 = np.float64


def n(t):
    return None if t is None else t.numpy()


def inject():
    worst = 0.0
    for case in T.INJ_CASES:
        N, D, nrows, last, o16, acc, zero = case
        dx, prior, row0 = T.inject_bwd_case(*case)
        rows = n(dx[:, row0:row0 + nrows])
        r64 = rows.astype(f64)
        t64, scale = r64.sum(0), np.abs(r64).sum(0)
        u = E.sum_error_units(E.inject_bwd_sum(rows), t64, scale)
        # the 16-group split against a plain serial sum over n, both fp32: another legal order
        serial = np.zeros(rows.shape[1:], np.float32)
        for k in range(N):
            serial = serial + rows[k].astype(np.float32)
        us = E.sum_error_units(serial, t64, scale)
        want = E.inject_bwd_out(rows, o16, n(prior))
        extra = 0.0
        if prior is not None:
            p64 = n(prior).astype(f64)
            extra = 0.5 * E.ulp(t64, 11) if o16 else E.ulp(np.abs(p64) + scale, 24)
            t64, scale = t64 + p64, scale + np.abs(p64)
        frac = E.check64(want, t64, scale, T.SUM_UNITS["inject"], extra, str(case))
        print(f"inject_bwd N={N:2d} D={D:3d} nrows={nrows} f16={int(o16)} acc={int(acc)}: grouped {u:.3f}, serial "
              f"{us:.3f} fp32 ulps of sum|terms|; output at {frac:.3f} of the test's fp64 tolerance")
        worst = max(worst, u)
    print(f"inject_bwd worst {worst:.3f}")
    return worst


def colsum():
    worst = 0.0
    for case in T.COLSUM_CASES:
        R, C, pad, lead, kind = case
        x = n(T.colsum_case(*case))
        x64 = x.astype(f64)
        t64, scale = x64.sum(0), np.abs(x64).sum(0)
        part = E.colsum_partials(x)
        assert part.shape == ((R + 63) // 64, C)
        u = E.sum_error_units(E.col_reduce(part), t64, scale)
        # the partials themselves: chunk b against the fp64 sum of its rows
        up = max(E.sum_error_units(part[b], x64[64 * b:64 * b + 64].sum(0), np.abs(x64[64 * b:64 * b + 64]).sum(0))
                 for b in range(part.shape[0]))
        frac = 0.0 if kind == "none" else E.check64(E.colsum(x, kind == "f16"), t64, scale, T.SUM_UNITS["colsum"], 0.0, str(case))
        print(f"colsum R={R:3d} C={C:3d} {kind:4s}: sum {u:.3f}, partials {up:.3f} fp32 ulps of sum|terms|; output at "
              f"{frac:.3f} of the test's fp64 tolerance")
        worst = max(worst, u, up)
    print(f"colsum worst {worst:.3f}")
    return worst


def linear():
    worst = dict(Y=0.0, dX=0.0, dW=0.0, db=0.0)
    flips = 0
    for case in T.SL_CASES:
        f16, M, I, O, bias, absent, acc = case
        c = {k: n(v) for k, v in T.small_linear_case(*case).items()}
        X64, W64, dY64 = (c[k].astype(f64) for k in ("X", "W", "dY"))
        Xf, Wf = c["X"].astype(np.float32), c["W"].astype(np.float32)
        y32 = E.wave_sum(E.lane_partials(Xf[:, None, :] * Wf[None, :, :]))
        u = dict(Y=E.sum_error_units(y32, X64 @ W64.T, T._mm_scale(c["X"], c["W"].T)),
                 dX=E.sum_error_units(E.small_linear_dx_sum(c["dY"], c["W"]), dY64 @ W64, T._mm_scale(c["dY"], c["W"])))
        # dW / db before their rounding: the serial loop over m in fp32
        dW32, db32 = np.zeros((O, I), np.float32), np.zeros(O, np.float32)
        dYf = c["dY"].astype(np.float32)
        for m in range(M):
            dW32 = dW32 + dYf[m][:, None] * Xf[m][None, :]
            db32 = db32 + dYf[m]
        u["dW"] = E.sum_error_units(dW32, dY64.T @ X64, T._mm_scale(c["dY"].T, c["X"]))
        u["db"] = E.sum_error_units(db32, dY64.sum(0), np.abs(dY64).sum(0))
        units = T.SUM_UNITS["linear"]
        dW, db = E.small_linear_dw_db(c["dY"], c["X"])
        E.check64(E.small_linear_fwd(c["X"], c["W"], None), X64 @ W64.T, T._mm_scale(c["X"], c["W"].T), units, 0.0, "Y")
        E.check64(E.small_linear_dx(c["dY"], c["W"]), dY64 @ W64, T._mm_scale(c["dY"], c["W"]), units, 0.0, "dX")
        E.check64(dW, dY64.T @ X64, T._mm_scale(c["dY"].T, c["X"]), units, 0.0, "dW")
        E.check64(db, dY64.sum(0), np.abs(dY64).sum(0), units, 0.0, "db")
        line = f"small_linear f16={int(f16)} M={M:2d} I={I:3d} O={O:3d}: " + ", ".join(f"{k} {v:.3f}" for k, v in u.items())
        if f16:  # where the restatement's fp16 output is not the rounded fp64 value (a sum on a rounding boundary)
            y = E.small_linear_fwd(c["X"], c["W"], None)
            d = int((y != (X64 @ W64.T).astype(np.float16)).sum()) + \
                int((E.small_linear_dx(c["dY"], c["W"]) != (dY64 @ W64).astype(np.float16)).sum())
            flips += d
            line += f"; {d} fp16 outputs differ from the rounded fp64 value"
        print(line + " (fp32 ulps of sum|terms|)")
        for k in worst:
            worst[k] = max(worst[k], u[k])
    print("small_linear worst " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) +
          f"; {flips} fp16 outputs on a rounding boundary in all")
    return max(worst.values())


def caption():
    worst = 0.0

    def moved(by):
        def exp(x):
            e = np.exp(x.astype(np.float32)).astype(np.float32)
            return np.nextafter(e, np.float32(np.inf if by > 0 else -np.inf)).astype(np.float32)
        return exp

    for B, Tn, D in T.CAPTION_CASES:
        tok, table, w = (n(t) for t in T.caption_case(B, Tn, D))
        ref64 = E.caption_pool64(tok, table, w)
        base = E.caption_pool(tok, table, w)
        u = [T._caption_units(base, ref64)]
        for by in (+1, -1):
            alt = E.caption_pool(tok, table, w, moved(by))
            u.append(T._caption_units(alt, ref64))
            u.append(T._caption_units(alt, base.astype(f64)))
        s64 = table[tok].astype(np.float16).astype(f64) @ w.astype(f64)
        sflip = int((E.caption_scores(tok, table, w) != s64.astype(np.float16).astype(np.float32)).sum())
        print(f"caption_pool B={B} T={Tn:3d} D={D:3d}: restatement vs fp64 {u[0]:.3f}; expf +1 ulp: {u[1]:.3f} vs fp64, "
              f"{u[2]:.3f} vs restatement; expf -1 ulp: {u[3]:.3f}, {u[4]:.3f} (fp16 ulps); {sflip} scores differ "
              "from the rounded fp64 score")
        worst = max(worst, *u)
    print(f"caption_pool worst {worst:.3f} fp16 ulps")
    return worst


if __name__ == "__main__":
    parts = sys.argv[1:] or ["inject", "colsum", "linear", "caption"]
    sums = [dict(inject=inject, colsum=colsum, linear=linear)[p]() for p in parts if p != "caption"]
    if sums:
        print(f"worst fp32 sum error of all families: {max(sums):.3f} fp32 ulps of sum|terms| "
              f"(SUM_UNITS = {T.SUM_UNITS})")
    if "caption" in parts:
        caption()
