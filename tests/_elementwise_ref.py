"""fp32 restatements (numpy, one rounding per operation) of the summation grouping of the kernels of
csrc/elementwise.hip, shared by tests/test_elementwise_kernels_gpu.py (compared bit for bit with the device) and
tests/diagnostics/elementwise_bounds.py (measured against fp64 on the CPU).  Arrays in, arrays out; fp16 operands are
numpy float16, every accumulation is float32 in the order the kernel uses."""
import numpy as np

f32 = np.float32
f16 = np.float16


def r16(x):
    """mf_common.h r16: fp32 -> fp16 (round to nearest even) -> fp32."""
    return np.asarray(x, f32).astype(f16).astype(f32)


def wave_sum(v):
    """wave_sum / wave_max's butterfly on [..., 64] lanes: xor 32, 16, .., 1; every lane ends with the same bits."""
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ o]
    return v[..., 0]


def lane_partials(terms):
    """terms [..., n] -> [..., 64]: lane l sums terms l, l + 64, ... in order, starting from 0.f."""
    n = terms.shape[-1]
    s = np.zeros(terms.shape[:-1] + (64,), f32)
    for i0 in range(0, n, 64):
        w = min(64, n - i0)
        s[..., :w] = s[..., :w] + terms[..., i0:i0 + w]
    return s


# ------------------------------------------------------------------------------------------ inject_bwd_kernel
def inject_bwd_sum(rows):
    """rows [N, nrows, D] fp16 (the injected rows of dx) -> t [nrows, D] fp32: wave group g sums n = g, g + 16, ...
    in order from 0.f, then red[0] + red[1] + ... + red[15]."""
    v = rows.astype(f32)
    N = v.shape[0]
    red = []
    for g in range(16):
        s = np.zeros(v.shape[1:], f32)
        for n in range(g, N, 16):
            s = s + v[n]
        red.append(s)
    t = red[0]
    for k in range(1, 16):
        t = t + red[k]
    return t


def inject_bwd_out(rows, out_f16, prior=None):
    """The value mf_prompt_inject_bwd leaves in out; prior: out's previous content when accumulate is set."""
    t = inject_bwd_sum(rows)
    if out_f16:
        return t.astype(f16) if prior is None else (prior.astype(f32) + r16(t)).astype(f16)
    return t if prior is None else prior.astype(f32) + t


# ------------------------------------------------------------------- colsum_part_kernel + col_reduce_kernel
def colsum_partials(x):
    """x [R, C] fp16 -> part [ceil(R / 64), C] fp32: wave w of chunk b sums rows 64 b + 16 w .. + 15 in order from
    0.f, then red[0] + red[1] + red[2] + red[3]."""
    v = x.astype(f32)
    R, C = v.shape
    nb = (R + 63) // 64
    part = np.zeros((nb, C), f32)
    for b in range(nb):
        red = []
        for w in range(4):
            r0 = b * 64 + w * 16
            s = np.zeros(C, f32)
            for r in range(r0, min(R, r0 + 16)):
                s = s + v[r]
            red.append(s)
        part[b] = ((red[0] + red[1]) + red[2]) + red[3]
    return part


def col_reduce(part):
    """mf_common.h col_reduce_kernel on part [nblk, C] -> [C] fp32 (before the output's rounding): group g sums
    blocks g, g + 16, ... into four accumulators 64 blocks apart, the tail into the first; (s0 + s1) + (s2 + s3);
    then the 16 groups in order from 0.f."""
    nblk, C = part.shape
    red = []
    for g in range(16):
        s = [np.zeros(C, f32) for _ in range(4)]
        b = g
        while b + 48 < nblk:
            for j in range(4):
                s[j] = s[j] + part[b + 16 * j]
            b += 64
        while b < nblk:
            s[0] = s[0] + part[b]
            b += 16
        red.append((s[0] + s[1]) + (s[2] + s[3]))
    t = np.zeros(C, f32)
    for k in range(16):
        t = t + red[k]
    return t


def colsum(x, out_f16):
    t = col_reduce(colsum_partials(x))
    return t.astype(f16) if out_f16 else t


# ------------------------------------------------------------------------------------------- small linears
def small_linear_fwd(X, W, b):
    """Y [M, O] of dtype X.dtype: lane-strided partials over i, the butterfly, plus bias (0.f without), one rounding."""
    Xf, Wf = X.astype(f32), W.astype(f32)
    s = wave_sum(lane_partials(Xf[:, None, :] * Wf[None, :, :]))
    bias = b.astype(f32)[None, :] if b is not None else f32(0)
    return (s + bias).astype(X.dtype)


def small_linear_dx_sum(dY, W):
    """s [M, I] fp32 of small_linear_bwd_dx_kernel: group g takes o = g, g + 32, ... into s0 and o = g + 16, g + 48,
    ... into s1 while o + 16 < O, the tail into s0; s0 + s1; then the 16 groups in order from 0.f."""
    dYf, Wf = dY.astype(f32), W.astype(f32)
    M, O = dYf.shape
    I = Wf.shape[1]
    t = np.zeros((M, I), f32)
    for g in range(16):
        s0, s1 = np.zeros((M, I), f32), np.zeros((M, I), f32)
        o = g
        while o + 16 < O:
            s0 = s0 + dYf[:, o:o + 1] * Wf[o][None, :]
            s1 = s1 + dYf[:, o + 16:o + 17] * Wf[o + 16][None, :]
            o += 32
        while o < O:
            s0 = s0 + dYf[:, o:o + 1] * Wf[o][None, :]
            o += 16
        t = t + (s0 + s1)
    return t


def small_linear_dx(dY, W, prior=None):
    """dX of dtype dY.dtype; prior: its previous content when accumulate_dx is set (the new term is rounded to the
    dtype once, then added)."""
    s = small_linear_dx_sum(dY, W)
    T = dY.dtype
    if prior is None:
        return s.astype(T)
    return (prior.astype(f32) + s.astype(T).astype(f32)).astype(T)


def small_linear_dw_db(dY, X):
    """dW [O, I], db [O] of dtype dY.dtype: serial loops over m from 0.f."""
    dYf, Xf = dY.astype(f32), X.astype(f32)
    M, O = dYf.shape
    dW = np.zeros((O, Xf.shape[1]), f32)
    db = np.zeros(O, f32)
    for m in range(M):
        dW = dW + dYf[m][:, None] * Xf[m][None, :]
        db = db + dYf[m]
    return dW.astype(dY.dtype), db.astype(dY.dtype)


# --------------------------------------------------------------------------------------- caption_pool_kernel
def caption_scores(tok, table, w):
    """s [B, T] fp32 (fp16 values): lane-strided partials of fp16(table[id]) * w over d, the butterfly, r16.  An id
    outside the table scores NaN."""
    vocab = table.shape[0]
    ok = (tok >= 0) & (tok < vocab)
    emb = table[np.where(ok, tok, 0)].astype(f16).astype(f32)          # [B, T, D]
    s = r16(wave_sum(lane_partials(emb * w.astype(f32)[None, None, :])))
    return np.where(ok, s, f32(np.nan)).astype(f32)


def caption_probs(s, exp=None):
    """p [B, T] fp32 (fp16 values) from the scores: max, lane-strided partials of expf(s - m), the butterfly,
    r16(expf(s - m) / z).  exp: the fp32 exponential to use (default numpy's)."""
    exp = exp or (lambda x: np.exp(x.astype(f32)).astype(f32))
    m = s.max(axis=1, keepdims=True)                                    # max is exact in any order; NaN propagates
    e = exp((s - m).astype(f32))
    z = wave_sum(lane_partials(e))
    return r16(e / z[:, None])


def caption_pool(tok, table, w, exp=None):
    """pooled [B, D] fp16: acc += r16(fp16(table[id]) * p[t]) over the tokens in order from 0.f, one rounding."""
    vocab = table.shape[0]
    ok = (tok >= 0) & (tok < vocab)
    emb = np.where(ok[..., None], table[np.where(ok, tok, 0)].astype(f16).astype(f32), f32(0))
    p = caption_probs(caption_scores(tok, table, w), exp)
    acc = np.zeros((tok.shape[0], table.shape[1]), f32)
    for t in range(tok.shape[1]):
        acc = acc + r16(emb[:, t, :] * p[:, t:t + 1])
    return acc.astype(f16)


def caption_pool64(tok, table, w):
    """The same computation in fp64 through the same fp16 rounding points (embedding, score, probability, each
    product, the result); valid ids only."""
    emb = table[tok].astype(f16).astype(np.float64)
    s = (emb @ w.astype(np.float64)).astype(f16).astype(np.float64)
    e = np.exp(s - s.max(axis=1, keepdims=True))
    p = (e / e.sum(axis=1, keepdims=True)).astype(f16).astype(np.float64)
    return (emb * p[..., None]).astype(f16).astype(np.float64).sum(axis=1)


# ------------------------------------------------------------------------------------------- fp64 comparison
def ulp(x, p):
    """Unit in the last place of |x| in a binary format of p significand bits (fp16: 11, clamped at its smallest
    normal 2^-14; fp32: 24)."""
    a = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** (-14 if p == 11 else -126))
    return np.exp2(np.floor(np.log2(a)) - (p - 1))


def sum_error_units(s32, ref64, scale64):
    """Largest |s32 - ref64| in fp32 ulps of scale64 (the sum of the terms' magnitudes): the figure
    elementwise_bounds.py prints for an fp32 sum before any rounding of the output."""
    return float((np.abs(s32.astype(np.float64) - ref64) / ulp(scale64, 24)).max()) if s32.size else 0.0


def check64(out, ref64, scale64, units, extra=0.0, what=""):
    """|out - ref64| <= units fp32 ulps of scale64 (the fp32 summation error allowed), plus half an fp16 ulp of
    ref64 when out is fp16 (its one rounding), plus `extra` (absolute; a second rounding).  Returns the worst
    error / tolerance."""
    tol = units * ulp(scale64, 24) + extra
    if out.dtype == f16:
        tol = tol + 0.5 * ulp(ref64, 11)
    err = np.abs(out.astype(np.float64) - ref64)
    worst = float((err / tol).max()) if err.size else 0.0
    assert worst <= 1.0, f"{what}: {worst:.3f} of the fp64 tolerance"
    return worst
