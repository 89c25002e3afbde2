"""The three reduction kernels between the GEMMs and the optimizer step, on every dispatch path, against fp64:
LayerNorm (csrc/layernorm.hip), the CLIP head and loss (csrc/head.hip) and the gradient-norm clip
(csrc/optim.hip sumsq_chunks_kernel / clip_coef_kernel).

Which input reaches which kernel form (read off the dispatch conditions of the entry points):

LayerNorm, D in {512, 768}
  contiguous, 16-byte aligned rows          mf_layernorm_fwd -> ln_fwd2_kernel (v16)
  rows 37 (3 row blocks), 4080 (255)        mf_layernorm_bwd -> ln_bwd2_kernel<D, 16>   (ln_bwd_wide: nblk < 256)
  rows 4081 (256 row blocks)                mf_layernorm_bwd -> ln_bwd2_kernel<D, 8>    (two rows per half-wave)
  leading dimension D + 8, aligned          the same kernels through their ld arguments (ld % 8 == 0 keeps v16)
  4 elements into an allocation, ld D + 4   pointer % 16 == 8 and ld % 8 == 4: v16 false -> ln_fwd_kernel /
                                            ln_bwd_kernel (wave per row, 8-byte accesses)
  mf_layernorm_fwd_inject, ldx = D + 8      ldx != D -> mf_prompt_inject_fwd_ld + mf_layernorm_fwd (ln_fwd2_kernel)
  row_index                                 the gather argument of ln_fwd2_kernel / ln_bwd2_kernel<D, 16>
  accumulate                                col_reduce_kernel's `*o + s` branch

CLIP head (B, K, D)
  every shape                               normalize_rows_kernel, logits_kernel, loss_kernel, dimg_kernel,
                                            dtxt_kernel, normalize_bwd_kernel (soft: soft_target_kernel,
                                            loss_soft_kernel, dtxt_soft_kernel)
  K = 38, 17, 10                            dimg_kernel: 2 / 1 / 0 unrolled 16-wide steps plus a 6 / 1 / 10 tail
  K = 1000                                  62 unrolled steps plus a tail of 8; loss_kernel's k loop runs 16 times
  K = 1                                     tail only; a one-element softmax
  B = 64                                    every slot of loss_kernel's s_ce / s_cos; rows wrap 4 times on 16 waves
  D = 96                                    dimg_kernel's second column block is half empty (d >= D returns after the
                                            wave reduction); the 256-thread kernels leave threads 96.. idle
  logit_scale log(200)                      the fminf(expf(.), 100) clamp
  label -1, K                               loss_kernel's y_bad path; dimg_kernel's row-0 stand-in
  B = 65                                    the B <= 64 guard of both loss entry points

Gradient-norm clip
  1024 chunks                               one full tile of clip_coef_kernel, no second pass
  1025 chunks                               a second tile whose first chunk starts a new segment
  the long table (about 2 760 chunks)       three tiles; the fp32 segment of 1100 chunks crosses the 2048 boundary
                                            (carry_val / carry_seg); odd segment starts run the scalar head and tail
                                            loops of sumsq_chunks_kernel around the 16-byte middle

Bounds that no earlier test sets come from tests/diagnostics/reduction_bounds.py, which restates the kernels'
arithmetic in fp32 on the CPU (same summation grouping) and measures it against fp64 on these very inputs; the
docstrings below quote what it printed, the margin, and what the MI355X gave.
"""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from federated_multi_modal_amd import _lib, ops
from test_kernels_gpu import assert_ulps, ulp16

pytestmark = pytest.mark.gpu

SENTINEL = -7.25  # exact in fp16; no kernel output below equals it by accident in a whole pad column


# ------------------------------------------------------------------------------------------------ LayerNorm

LN_D = (512, 768)
LN_ROWS = (37, 4080, 4081)

# |mean - mean64| <= LN_MEAN_BOUND * mean_j |x_j| and |rstd - rstd64| <= LN_RSTD_BOUND * rstd64, per row.
# reduction_bounds.py (fp32 restatement of ln_fwd2_kernel vs fp64, worst over D x rows of LN_D x LN_ROWS and the
# edge rows of _ln_edge_rows): mean 4.62e-8, rstd 1.43e-7; 4x margin for another legal fp32 summation order.
# MI355X: the same figures, 4.62e-8 and 1.43e-7, case by case (the restatement is the kernel, bit for bit).
LN_MEAN_BOUND = 4 * 4.62e-8
LN_RSTD_BOUND = 4 * 1.43e-7


def _ln_case_host(D, rows):
    g = torch.Generator().manual_seed(1000 * D + rows)
    x = (torch.randn(rows, D, generator=g) * 2 + 0.5).half()
    gamma = 1 + 0.1 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    dy = torch.randn(rows, D, generator=g).half()
    dres = torch.randn(rows, D, generator=g).half()
    return x, gamma, beta, dy, dres


def _ln_ref64(x, gamma, beta, dy):
    """fp64 LayerNorm forward and autograd backward of fp16 / fp32 inputs, on the inputs' device."""
    D = x.shape[1]
    xx = x.double().requires_grad_(True)
    gg = gamma.double().requires_grad_(True)
    bb = beta.double().requires_grad_(True)
    y = F.layer_norm(xx, (D,), gg, bb, 1e-5)
    y.backward(dy.double())
    xd = x.double()
    mean = xd.mean(1)
    rstd = 1.0 / torch.sqrt(xd.var(1, unbiased=False) + float(np.float32(1e-5)))
    return dict(y=y.detach(), mean=mean, rstd=rstd, dx=xx.grad, dgamma=gg.grad, dbeta=bb.grad,
                absmean=xd.abs().mean(1))


@functools.lru_cache(maxsize=None)
def _ln_case(D, rows):
    """Inputs on the GPU and their fp64 reference, computed once per (D, rows) and never written to."""
    dev = torch.device("cuda:0")
    x, gamma, beta, dy, dres = (t.to(dev) for t in _ln_case_host(D, rows))
    return dict(x=x, gamma=gamma, beta=beta, dy=dy, dres=dres, ref=_ln_ref64(x, gamma, beta, dy))


def _check_stats(mean, rstd, ref, what):
    em = ((mean.double() - ref["mean"]).abs() - LN_MEAN_BOUND * ref["absmean"]).max().item()
    er = ((rstd.double() - ref["rstd"]).abs() / ref["rstd"]).max().item()
    wm = ((mean.double() - ref["mean"]).abs() / ref["absmean"].clamp_min(1e-30)).max().item()
    print(f"{what}: mean err / mean|x| {wm:.3e} (bound {LN_MEAN_BOUND:.3e}), rstd rel err {er:.3e} "
          f"(bound {LN_RSTD_BOUND:.3e})")
    assert em <= 0, f"{what}: mean off by {wm:.3e} of mean|x|"
    assert er <= LN_RSTD_BOUND, f"{what}: rstd rel err {er:.3e}"


def _check_dx(dx, refdx, what):
    """test_layernorm's bound: 2 fp16 ulps of the largest reference value."""
    err = (dx.double() - refdx).abs().max().item()
    assert err <= 2 * ulp16(refdx).max().item(), f"{what}: dx err {err:.3e}"


def _check_dgb(dg, db, ref, what):
    """test_layernorm's bound."""
    torch.testing.assert_close(dg.double(), ref["dgamma"], rtol=1e-4, atol=1e-3, msg=lambda m: f"{what} dgamma: {m}")
    torch.testing.assert_close(db.double(), ref["dbeta"], rtol=1e-4, atol=1e-3, msg=lambda m: f"{what} dbeta: {m}")


def _strided(t, pad, lead=0):
    """A copy of the 2-D tensor t as a view with leading dimension cols + pad that starts `lead` elements into
    its allocation, the pad columns (and the lead) filled with SENTINEL.  Returns (view, whole padded rows)."""
    rows, cols = t.shape
    buf = torch.full((lead + rows * (cols + pad),), SENTINEL, dtype=t.dtype, device=t.device)
    full = buf[lead:].view(rows, cols + pad)
    full[:, :cols] = t
    return full[:, :cols], full


def _ln_run(c, pad=0, lead=0, with_dres=True):
    """Forward and backward of case c in the given layout (every fp16 operand laid out alike)."""
    D = c["x"].shape[1]
    rows = c["x"].shape[0]
    dev = c["x"].device
    x, _ = _strided(c["x"], pad, lead)
    dy, _ = _strided(c["dy"], pad, lead)
    y, yfull = _strided(torch.zeros_like(c["x"]), pad, lead)
    dx, dxfull = _strided(torch.zeros_like(c["x"]), pad, lead)
    dres = _strided(c["dres"], pad, lead)[0] if with_dres else None
    mean = torch.empty(rows, device=dev)
    rstd = torch.empty(rows, device=dev)
    ops.layernorm_fwd(x, c["gamma"], c["beta"], y, mean, rstd)
    dg, db = torch.empty(D, device=dev), torch.empty(D, device=dev)
    ops.layernorm_bwd(dy, x, c["gamma"], mean, rstd, dx, dg, db, dres=dres)
    return dict(y=y, mean=mean, rstd=rstd, dx=dx, dg=dg, db=db, yfull=yfull, dxfull=dxfull)


@pytest.mark.parametrize("rows", LN_ROWS)
@pytest.mark.parametrize("D", LN_D)
def test_layernorm_every_output_fast_path(dev, D, rows):
    """ln_fwd2_kernel and both ln_bwd2_kernel forms: y, mean, rstd, dx (alone, with a residual gradient, and with
    the residual gradient aliasing dx as the engine passes it), dgamma and dbeta against fp64.  y, dx, dgamma and
    dbeta at test_layernorm's bounds; mean and rstd at LN_MEAN_BOUND / LN_RSTD_BOUND (see there)."""
    c = _ln_case(D, rows)
    ref = c["ref"]
    r = _ln_run(c)
    assert_ulps(r["y"], ref["y"], 1.0, 1e-2, "ln fwd")
    _check_stats(r["mean"], r["rstd"], ref, f"ln fwd D={D} rows={rows}")
    refdx16 = ref["dx"].half().double()
    _check_dx(r["dx"], c["dres"].double() + refdx16, "dx + dres")
    _check_dgb(r["dg"], r["db"], ref, "with dres")
    plain = _ln_run(c, with_dres=False)
    _check_dx(plain["dx"], ref["dx"], "dx")
    _check_dgb(plain["dg"], plain["db"], ref, "without dres")
    assert torch.equal(plain["dg"], r["dg"]) and torch.equal(plain["db"], r["db"])
    # dres aliasing dx
    acc = c["dres"].clone()
    dg, db = torch.empty(D, device=dev), torch.empty(D, device=dev)
    ops.layernorm_bwd(c["dy"], c["x"], c["gamma"], r["mean"], r["rstd"], acc, dg, db, dres=acc)
    assert torch.equal(acc, r["dx"]) and torch.equal(dg, r["dg"]) and torch.equal(db, r["db"])


@pytest.mark.parametrize("rows", LN_ROWS)
@pytest.mark.parametrize("D", LN_D)
def test_layernorm_fallback_and_strided_match_fast_path(dev, D, rows):
    """The wave-per-row kernels (operands 8 bytes into their allocations, leading dimension D + 4) give y, mean,
    rstd and dx bit for bit as the half-wave kernels do: a 16-byte chunk of half-wave lane hl holds the 4-element
    groups of wave lanes 2 hl and 2 hl + 1, kept as two partials whose 32-lane butterflies are the wave's xor
    32..2 steps and whose final sum is its xor-1 step.  Their dgamma / dbeta partials group rows differently
    (4 waves x 4 rows against 8 or 16 half-waves), so those are held to fp64 at test_layernorm's bounds.  The
    half-wave kernels at leading dimension D + 8 give the contiguous result and leave the pad columns alone."""
    c = _ln_case(D, rows)
    fast = _ln_run(c)
    slow = _ln_run(c, pad=4, lead=4)
    for k in ("y", "mean", "rstd", "dx"):
        assert torch.equal(slow[k], fast[k]), f"fallback {k} differs from the half-wave kernel's"
    _check_dgb(slow["dg"], slow["db"], c["ref"], "fallback")
    wide = _ln_run(c, pad=8)
    for k in ("y", "mean", "rstd", "dx", "dg", "db"):
        assert torch.equal(wide[k], fast[k]), f"ld D+8 {k} differs from the contiguous result"
    for r in (slow, wide):
        assert (r["yfull"][:, D:] == SENTINEL).all() and (r["dxfull"][:, D:] == SENTINEL).all()


@pytest.mark.parametrize("D", LN_D)
def test_layernorm_fwd_inject_strided_x(dev, D):
    """mf_layernorm_fwd_inject with ldx = D + 8 takes its two-kernel path; x, y, mean and rstd equal
    prompt_inject_fwd + layernorm_fwd on contiguous rows, and the pad columns of x stay as they were."""
    N, L, row0, nrows = 3, 7, 5, 2
    g = torch.Generator().manual_seed(D + L)
    x0 = torch.randn(N * L, D, generator=g).half().to(dev)
    prompt = torch.randn(nrows, D, generator=g).to(dev)
    gamma, beta = torch.randn(D, generator=g).to(dev), torch.randn(D, generator=g).to(dev)
    x1 = x0.clone()
    ops.prompt_inject_fwd(x1, prompt, N, L, row0, nrows, D)
    y1, m1, r1 = ops.layernorm_fwd(x1, gamma, beta)
    assert not torch.equal(x1, x0)
    x2, x2full = _strided(x0, 8)
    y2 = torch.empty_like(y1)
    m2, r2 = torch.empty_like(m1), torch.empty_like(r1)
    ops.layernorm_fwd_inject(x2, gamma, beta, y2, m2, r2, prompt, L, row0, nrows)
    assert torch.equal(x2, x1), "injected rows of a strided x"
    assert (x2full[:, D:] == SENTINEL).all()
    assert torch.equal(y2, y1) and torch.equal(m2, m1) and torch.equal(r2, r1)


@pytest.mark.parametrize("D", LN_D)
def test_layernorm_bwd_wide_and_two_row_partials_identical(dev, D):
    """Rows 0..4079 as a 4080-row call (255 blocks, one row per half-wave) and inside the 4081-row call (256
    blocks, two rows per half-wave): the first 255 blocks' dgamma / dbeta partials, read from the workspace
    ([dgamma partials | dbeta partials], nblk x D each), and the dx rows are bit-identical."""
    c = _ln_case(D, 4081)
    x, dy, gamma = c["x"], c["dy"], c["gamma"]
    _, mean, rstd = ops.layernorm_fwd(x, gamma, c["beta"])
    out = {}
    for rows in (4080, 4081):
        nblk = (rows + 15) // 16
        assert ops.layernorm_ws_floats(rows, D) == 2 * nblk * D
        ws = torch.full((2 * nblk * D,), float("nan"), device=dev)
        dx = torch.zeros(rows, D, dtype=torch.float16, device=dev)
        dg, db = torch.empty(D, device=dev), torch.empty(D, device=dev)
        ops.layernorm_bwd(dy[:rows], x[:rows], gamma, mean[:rows], rstd[:rows], dx, dg, db, workspace=ws)
        out[rows] = (ws.view(2, nblk, D), dx)
    (w0, dx0), (w1, dx1) = out[4080], out[4081]
    assert torch.isfinite(w0).all() and torch.isfinite(w1).all()
    assert torch.equal(w0[0], w1[0, :255]) and torch.equal(w0[1], w1[1, :255])
    assert torch.equal(dx0, dx1[:4080])


@pytest.mark.parametrize("D", LN_D)
def test_layernorm_row_index_bwd_values(dev, D):
    """The gathered backward: dx at the indexed rows, dgamma and dbeta against fp64 autograd of
    layer_norm(x[idx]); every other row of a pre-filled dx is untouched."""
    L, N = 199, 4
    g = torch.Generator().manual_seed(D + 1)
    x = (torch.randn(N * L, D, generator=g) * 2 + 0.5).half().to(dev)
    idx = torch.tensor([5, L + 198, 2 * L + 77, 3 * L + 1], dtype=torch.int32, device=dev)
    gamma = (1 + 0.1 * torch.randn(D, generator=g)).to(dev)
    beta = (0.1 * torch.randn(D, generator=g)).to(dev)
    dy = torch.randn(N, D, generator=g).half().to(dev)
    y, mean, rstd = ops.layernorm_fwd(x, gamma, beta, row_index=idx)
    ref = _ln_ref64(x[idx.long()], gamma, beta, dy)
    assert_ulps(y, ref["y"], 1.0, 1e-2, "ln gather")
    _check_stats(mean, rstd, ref, "ln gather")
    dx = torch.full_like(x, SENTINEL)
    dg, db = torch.empty(D, device=dev), torch.empty(D, device=dev)
    ops.layernorm_bwd(dy, x, gamma, mean, rstd, dx, dg, db, row_index=idx)
    _check_dx(dx[idx.long()], ref["dx"], "gathered dx")
    _check_dgb(dg, db, ref, "gathered")
    mask = torch.ones(N * L, dtype=torch.bool, device=dev)
    mask[idx.long()] = False
    assert (dx[mask] == SENTINEL).all()


@pytest.mark.parametrize("D,rows", [(512, 37), (768, 4081)])
def test_layernorm_bwd_accumulate(dev, D, rows):
    """accumulate=True adds the column sums to what dgamma / dbeta hold: bit for bit prefill + the
    accumulate=False result, formed in fp32 on the device."""
    c = _ln_case(D, rows)
    _, mean, rstd = ops.layernorm_fwd(c["x"], c["gamma"], c["beta"])
    dx = torch.empty_like(c["x"])
    dg0, db0 = torch.empty(D, device=dev), torch.empty(D, device=dev)
    ops.layernorm_bwd(c["dy"], c["x"], c["gamma"], mean, rstd, dx, dg0, db0)
    g = torch.Generator().manual_seed(3)
    pg, pb = torch.randn(D, generator=g).to(dev) * 10, torch.randn(D, generator=g).to(dev) * 10
    dg, db = pg.clone(), pb.clone()
    ops.layernorm_bwd(c["dy"], c["x"], c["gamma"], mean, rstd, dx, dg, db, accumulate=True)
    assert torch.equal(dg, pg + dg0) and torch.equal(db, pb + db0)


EDGE_ZERO, EDGE_CONST, EDGE_OFFSET, EDGE_OUTLIER, EDGE_HUGE = 0, 1, 2, 3, 4

# |dx - dx64| <= LN_EDGE_DX_BOUND fp16 ulps of the row's largest |dx64|, for the offset row (30 + 0.5 randn, where
# b = (sum(dg) mean - sum(dg x)) rstd^3 / D loses digits to cancellation) and the outlier row.  reduction_bounds.py
# (fp32 restatement of ln_bwd2_kernel's b / c formula with fp16 output, vs fp64): offset row 0.490 (D = 512) and 0.488
# (768), outlier row 0.497 and 0.492 ulps: the output's own fp16 rounding, half an ulp at the row maximum.  The
# cancellation leaves b a relative error of 6.4e-6 (offset row) and 2.6e-7 (outlier row), far below that rounding.
# 4x the worst is 1.99, test_layernorm's 2 ulps in effect; the remaining rows keep those.
# MI355X: the same four figures.
LN_EDGE_DX_BOUND = 4 * 0.497


def _ln_edge_rows(D):
    g = torch.Generator().manual_seed(77 + D)
    x = torch.randn(16, D, generator=g)
    x[EDGE_ZERO] = 0.0
    x[EDGE_CONST] = 3.0
    x[EDGE_OFFSET] = 30 + 0.5 * torch.randn(D, generator=g)
    x[EDGE_OUTLIER, D // 3] = 1000.0
    x[EDGE_HUGE] = 65504.0 * (1 - 2 * (torch.arange(D) % 2)).float()
    gamma = 1 + 0.1 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    dy = torch.randn(16, D, generator=g).half()
    return x.half(), gamma, beta, dy


@pytest.mark.parametrize("D", LN_D)
def test_layernorm_edge_rows(dev, D):
    """A zero row, a constant row, a row with |mean| = 60 std, a row with one channel at 1000 and a row of
    alternating +-65504 among ordinary rows.  Forward: a row whose elements all equal its mean gives
    x rstd + (-rstd mean) = 0 exactly, so y = fp16(beta), and rstd = fp32(1 / sqrt(1e-5)) to one fp32 ulp; the
    rest against fp64 at test_layernorm's bound, mean / rstd at LN_MEAN_BOUND / LN_RSTD_BOUND.  Backward: dx of
    every row against fp64, per row, the offset and the outlier row at LN_EDGE_DX_BOUND (see there), the others
    at test_layernorm's 2 ulps of the row's largest value."""
    x, gamma, beta, dy = (t.to(dev) for t in _ln_edge_rows(D))
    ref = _ln_ref64(x, gamma, beta, dy)
    y, mean, rstd = ops.layernorm_fwd(x, gamma, beta)
    for r in (EDGE_ZERO, EDGE_CONST):
        assert torch.equal(y[r], beta.half()), f"row {r}: y != fp16(beta)"
        assert mean[r].item() == x[r, 0].item()
    r0 = np.float32(1.0) / np.sqrt(np.float32(1e-5))
    assert (rstd[[EDGE_ZERO, EDGE_CONST]].cpu().numpy() - r0 <= np.spacing(r0)).all()
    assert (r0 - rstd[[EDGE_ZERO, EDGE_CONST]].cpu().numpy() <= np.spacing(r0)).all()
    assert_ulps(y, ref["y"], 1.0, 1e-2, "ln edge rows fwd")
    _check_stats(mean, rstd, ref, f"ln edge rows D={D}")
    dx = torch.empty_like(x)
    dg, db = torch.empty(D, device=dev), torch.empty(D, device=dev)
    ops.layernorm_bwd(dy, x, gamma, mean, rstd, dx, dg, db)
    assert torch.isfinite(dx).all()
    unit = ulp16(ref["dx"].abs().max(1).values)
    ulps = (dx.double() - ref["dx"]).abs().max(1).values / unit
    print(f"ln edge rows D={D}: dx err in fp16 ulps of the row maximum {[round(v, 3) for v in ulps.tolist()]}")
    bound = torch.full_like(ulps, 2.0)
    bound[[EDGE_OFFSET, EDGE_OUTLIER]] = LN_EDGE_DX_BOUND
    assert (ulps <= bound).all(), ulps.tolist()
    # dbeta sums dy alone; dgamma's reference is ill-conditioned only through xhat, which fp64 forms exactly enough
    torch.testing.assert_close(db.double(), ref["dbeta"], rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(dg.double(), ref["dgamma"], rtol=1e-4, atol=1e-3)


# ------------------------------------------------------------------------------------------- CLIP head and loss

HEAD_SHAPES = [(8, 38, 512), (1, 1, 512), (64, 38, 512), (5, 17, 512), (3, 1000, 512), (4, 10, 96)]
HEAD_SOFT_SHAPES = [(8, 38, 512), (3, 1000, 512)]
HEAD_SOFT_B64 = (64, 10, 512)
HEAD_SHARED = (8, 6, 512)
HEAD_SHARED_LABELS = ([2, 2, 2, 0, 1, 3, 5, 5], [3] * 8)
HEAD_ZERO_ROW = (4, 10, 512)

# The seed of every stage-checked case, keyed (shape, soft, labels).  A stage's fp64 reference and an fp32 evaluation
# of it legitimately round some element the other way when its value lies on an fp16 rounding boundary to within the
# fp32 summation error (about one element in a thousand), and where two fp16 roundings are stacked (dimg_n, dtxt_n:
# fp16(fp16(s) + fp16(c))) such a flip can grow to 2 ulps; in a buffer of fewer than 100 elements one flip alone
# exceeds the 1 % cap.  These are the first seeds for which the fp32 restatement stays under the bound in four
# different summation orders (tests/diagnostics/reduction_bounds.py head-search), i.e. cases without such an element.
HEAD_SEEDS = {((64, 38, 512), False, None): 2}


def head_seed(shape, soft=False, labels=None):
    return HEAD_SEEDS.get((shape, soft, labels), 1)


def _r16(t):
    return t.half().to(t.dtype)


def _f32(v, T, like):
    """The fp32 constant v as a 0-d tensor of dtype T."""
    return torch.tensor(float(np.float32(v)), dtype=T, device=like.device)


def _scale(ls):
    """min(exp(logit_scale), 100) in fp32, on logit_scale's device."""
    return ls.float().exp().clamp(max=100.0)


# The stage references: each takes the tensors the kernel read (its own earlier outputs among them) and restates one
# kernel with head.hip's rounding points, in dtype T.  T = float64 is the reference; T = float32 on the CPU is the
# restatement that reduction_bounds.py holds against it.

def ref_norms(x, T):
    return _r16((x.to(T) ** 2).sum(1).sqrt()).clamp_min(_f32(1e-8, T, x))


def ref_normalized(x, norms, T):
    return (x.to(T) / norms.to(T)[:, None]).half()


def ref_mm(img_n, txt_n, T):
    return (img_n.to(T) @ txt_n.to(T).t()).half()


def _log_probs(logits, T):
    lr = logits.to(T)
    mx = lr.max(1, keepdim=True).values
    lse = (lr - mx).exp().sum(1, keepdim=True).log()
    return _r16(lr - mx - lse)


def _cosine(a, t, T):
    """loss_kernel's cosine of the rows of a and t: (nu, nv, fp16 cos, fp16(a / nu))."""
    tiny = _f32(1e-8, T, a)
    nu = _r16((a ** 2).sum(1).sqrt()).clamp_min(tiny)
    nv = _r16((t ** 2).sum(1).sqrt()).clamp_min(tiny)
    a1, t1 = _r16(a / nu[:, None]), _r16(t / nv[:, None])
    return nu, nv, _r16(_r16(a1 * t1).sum(1)), a1


def ref_loss_hard(logits, img_n, txt_n, label, sc, T):
    B, K = logits.shape
    logp = _log_probs(logits, T)
    g = _r16(_f32(np.float32(-1.0) / np.float32(B), T, logits))
    dl = _r16(F.one_hot(label, K).to(T) * g - logp.exp() * g)
    dmm = (dl * sc.to(T)).half()
    nu, nv, c, _ = _cosine(img_n.to(T), txt_n[label].to(T), T)
    ce = _r16(-logp[torch.arange(B, device=logits.device), label].sum() / B)
    align = _r16(1 - _r16(c.sum() / B))
    total = _r16(ce + _r16(0.5 * align))
    return dict(dmm=dmm, cos_ws=torch.stack([nu, nv], 1).reshape(-1), loss=torch.stack([total, ce, align]))


def _dcos(B, T, like):
    return _r16(_f32(np.float32(-0.5) / np.float32(B), T, like))


def ref_dimg_n(dmm, img_n, txt_n, trow, cos_ws, T):
    B = img_n.shape[0]
    dcos = _dcos(B, T, img_n)
    nu, nv = cos_ws.to(T)[0::2, None], cos_ws.to(T)[1::2, None]
    s = _r16(dmm.to(T) @ txt_n.to(T))
    v = _r16(trow.to(T) / nv)
    a = img_n.to(T)
    dotp = (dcos * v * a).sum(1, keepdim=True)
    cosg = dcos * v / nu - a * dotp / (nu * nu * nu)
    return (s + _r16(cosg)).half()


def ref_dtxt_n(dmm, img_n, txt_n, label, cos_ws, T):
    B, K = dmm.shape
    dcos = _dcos(B, T, img_n)
    nu, nv = cos_ws.to(T)[0::2, None], cos_ws.to(T)[1::2, None]
    s = _r16(dmm.to(T).t() @ img_n.to(T))
    u = _r16(img_n.to(T) / nu)
    t = txt_n[label].to(T)
    dots = (dcos * u * t).sum(1, keepdim=True)
    cgb = dcos * u / nv - t * dots / (nv * nv * nv)
    cg = torch.zeros_like(s).index_add_(0, label, cgb)
    return (s + torch.where(cg != 0, _r16(cg), torch.zeros_like(cg))).half()


def ref_normalize_bwd(x, dy, norms, T):
    x, dy, n = x.to(T), dy.to(T), norms.to(T)[:, None]
    s = (dy * x).sum(1, keepdim=True)
    return (dy / n - x * s / (n * n * n)).half()


def ref_soft_target(q, txt_n, T):
    return (_r16(q.to(T)) @ txt_n.to(T)).half()


def ref_loss_soft(logits, img_n, tgt, q, sc, T):
    B, K = logits.shape
    logp = _log_probs(logits, T)
    invB = _f32(np.float32(1.0) / np.float32(B), T, logits)
    t = q.to(T).clamp_min(_f32(1e-8, T, logits))
    kl = (t * (t.log() - logp)).sum() / B
    g = _r16(-t * invB)
    dl = _r16(g - logp.exp() * g.sum(1, keepdim=True))
    dmm = (dl * sc.to(T)).half()
    dcos = _r16(_f32(np.float32(-0.5) * (np.float32(1.0) / np.float32(B)), T, logits))
    tr = tgt.to(T)
    nu, nv, c, a1 = _cosine(img_n.to(T), tr, T)
    dotp = (dcos * a1 * tr).sum(1, keepdim=True)
    gtgt = (dcos * a1 / nv[:, None] - tr * dotp / (nv * nv * nv)[:, None]).half()
    align = _r16(1 - _r16(c.sum() / B))
    total = kl + _r16(0.5 * align)
    return dict(dmm=dmm, gtgt=gtgt, cos_ws=torch.stack([nu, nv], 1).reshape(-1), loss=torch.stack([total, kl, align]))


def ref_dtxt_soft(dmm, img_n, q, gtgt, T):
    s = _r16(dmm.to(T).t() @ img_n.to(T))
    cg = _r16(_r16(q.to(T)).t() @ gtgt.to(T))
    return (s + cg).half()


def head_inputs(B, K, D, seed):
    """Host inputs of a head case: img, txt (fp16), labels, soft labels, logit_scale."""
    g = torch.Generator().manual_seed(1000 * seed + 100 * B + K + D)
    img = torch.randn(B, D, generator=g).half()
    txt = torch.randn(K, D, generator=g).half()
    label = torch.randint(0, K, (B,), generator=g)
    q = torch.rand(B, K, generator=g) ** 4
    q[0] = 0.0
    q[0, K // 2] = 1.0
    q = (q / q.sum(1, keepdim=True)).contiguous()
    return img, txt, label, q, torch.tensor([math.log(1 / 0.07)])


def _head_buffers(dev, B, K, D, fill=None):
    def mk(*shape, dtype=torch.float16):
        if fill is None:
            return torch.empty(*shape, dtype=dtype, device=dev)
        return torch.full(shape, fill, dtype=dtype, device=dev)
    return dict(img_n=mk(B, D), txt_n=mk(K, D), norms=mk(B + K, dtype=torch.float32), mm=mk(B, K), logits=mk(B, K),
                dmm=mk(B, K), cos_ws=mk(2 * B, dtype=torch.float32), loss=mk(4, dtype=torch.float32),
                dimg_n=mk(B, D), dtxt_n=mk(K, D), dimg=mk(B, D), dtxt=mk(K, D), soft_ws=mk(2 * B * D))


def _head_fwd(h):
    ops.clip_head_fwd(h["img"], h["txt"], h["ls"], h["img_n"], h["txt_n"], h["norms"], h["mm"], h["logits"])


def _head_hard(h, label):
    ops.clip_loss_fwd_bwd(h["img"], h["txt"], h["img_n"], h["txt_n"], h["norms"], h["logits"], label, h["ls"],
                          h["dmm"], h["cos_ws"], h["loss"], h["dimg_n"], h["dtxt_n"], h["dimg"], h["dtxt"])


def _head_soft(h, q):
    ops.clip_loss_soft_fwd_bwd(h["img"], h["txt"], h["img_n"], h["txt_n"], h["norms"], h["logits"], q, h["ls"],
                               h["dmm"], h["cos_ws"], h["soft_ws"], h["loss"], h["dimg_n"], h["dtxt_n"], h["dimg"],
                               h["dtxt"])


def _head(dev, shape, soft=False, labels=None, ls=None, zero_row=None):
    """Buffers and inputs of a head case on the device, after the forward."""
    img, txt, label, q, ls0 = head_inputs(*shape, head_seed(shape, soft, tuple(labels) if labels else None))
    if labels:
        label = torch.tensor(labels)
    if zero_row is not None:
        img[zero_row] = 0.0
    h = _head_buffers(dev, *shape)
    h.update(img=img.to(dev), txt=txt.to(dev), label=label.to(dev), q=q.to(dev),
             ls=(ls0 if ls is None else torch.tensor([ls])).to(dev))
    _head_fwd(h)
    return h


def _ulps(out, ref, max_ulp=1.0, frac=1e-2, what="", floor=2e-5):
    """assert_ulps, after printing the two figures it asserts on."""
    unit = torch.maximum(ulp16(ref), torch.tensor(floor * ref.abs().max().item(), device=ref.device))
    d = (out.float() - ref.float()).abs() / unit
    print(f"  {what}: worst {d.max().item():.2f} ulp, {(d > 0.51).float().mean().item():.4f} beyond half an ulp "
          f"({d.numel()} elements)")
    assert_ulps(out, ref, max_ulp, frac, what, floor)


def check_forward_stages(h, T, check=_ulps):
    B = h["img"].shape[0]
    check(h["norms"], ref_norms(torch.cat([h["img"], h["txt"]]), T), 1.0, what="norms")
    check(h["img_n"], ref_normalized(h["img"], h["norms"][:B], T), 1.0, what="img_n")
    check(h["txt_n"], ref_normalized(h["txt"], h["norms"][B:], T), 1.0, what="txt_n")
    check(h["mm"], ref_mm(h["img_n"], h["txt_n"], T), 1.0, what="mm")


def check_hard_stages(h, T, check=_ulps):
    B = h["img"].shape[0]
    r = ref_loss_hard(h["logits"], h["img_n"], h["txt_n"], h["label"], _scale(h["ls"]), T)
    check(h["dmm"], r["dmm"], 1.0, what="dmm")
    check(h["cos_ws"], r["cos_ws"], 1.0, what="cos_ws")
    check(h["loss"][:3], r["loss"], 1.0, what="loss[0..2]")
    check(h["dimg_n"], ref_dimg_n(h["dmm"], h["img_n"], h["txt_n"], h["txt_n"][h["label"]], h["cos_ws"], T), 1.0,
          what="dimg_n")
    check(h["dtxt_n"], ref_dtxt_n(h["dmm"], h["img_n"], h["txt_n"], h["label"], h["cos_ws"], T), 1.0, what="dtxt_n")
    check(h["dimg"], ref_normalize_bwd(h["img"], h["dimg_n"], h["norms"][:B], T), 1.0, what="dimg")
    check(h["dtxt"], ref_normalize_bwd(h["txt"], h["dtxt_n"], h["norms"][B:], T), 1.0, what="dtxt")


def check_soft_stages(h, T, check=_ulps):
    B, D = h["img"].shape
    tgt, gtgt = h["soft_ws"][:B * D].view(B, D), h["soft_ws"][B * D:2 * B * D].view(B, D)
    check(tgt, ref_soft_target(h["q"], h["txt_n"], T), 1.0, what="soft target")
    r = ref_loss_soft(h["logits"], h["img_n"], tgt, h["q"], _scale(h["ls"]), T)
    check(h["dmm"], r["dmm"], 1.0, what="soft dmm")
    check(gtgt, r["gtgt"], 1.0, what="soft target gradient")
    check(h["cos_ws"], r["cos_ws"], 1.0, what="soft cos_ws")
    check(h["loss"][:3], r["loss"], 1.0, what="soft loss[0..2]")
    check(h["dimg_n"], ref_dimg_n(h["dmm"], h["img_n"], h["txt_n"], tgt, h["cos_ws"], T), 1.0, what="soft dimg_n")
    check(h["dtxt_n"], ref_dtxt_soft(h["dmm"], h["img_n"], h["q"], gtgt, T), 1.0, what="soft dtxt_n")
    check(h["dimg"], ref_normalize_bwd(h["img"], h["dimg_n"], h["norms"][:B], T), 1.0, what="soft dimg")
    check(h["dtxt"], ref_normalize_bwd(h["txt"], h["dtxt_n"], h["norms"][B:], T), 1.0, what="soft dtxt")


def _formula64(h, soft):
    """fp64 autograd of the plain formula: normalize, scaled logits, CE (or KL) + 0.5 (1 - mean cos)."""
    i64 = h["img"].double().requires_grad_(True)
    t64 = h["txt"].double().requires_grad_(True)
    a = F.normalize(i64, dim=-1, eps=1e-8)
    t = F.normalize(t64, dim=-1, eps=1e-8)
    lg = _scale(h["ls"]).double() * (a @ t.t())
    if soft:
        q = h["q"].double()
        main = F.kl_div(F.log_softmax(lg, dim=1), q.clamp(min=1e-8), reduction="batchmean")
        tot = main + 0.5 * (1 - F.cosine_similarity(a, q @ t).mean())
    else:
        main = F.cross_entropy(lg, h["label"])
        tot = main + 0.5 * (1 - F.cosine_similarity(a, t[h["label"]]).mean())
    tot.backward()
    return tot.item(), main.item(), i64.grad, t64.grad


def _check_end_to_end(h, soft):
    """test_clip_head_loss's tolerances, against fp64."""
    tot, main, gi, gt = _formula64(h, soft)
    loss = h["loss"].cpu()
    assert loss[3].item() == 0.0
    assert abs(loss[0].item() - tot) < 5e-3, (loss[0].item(), tot)
    assert abs(loss[1].item() - main) < 5e-3, (loss[1].item(), main)
    torch.testing.assert_close(h["dimg"].double(), gi, rtol=2e-2, atol=2e-4)
    torch.testing.assert_close(h["dtxt"].double(), gt, rtol=2e-2, atol=2e-4)


@pytest.mark.parametrize("B,K,D", HEAD_SHAPES)
def test_clip_head_stages(dev, B, K, D):
    """Every buffer of the head and the hard-label loss, stage by stage: each stage's fp64 reference is fed the
    kernel's own earlier outputs, so it differs from the kernel by one fp16 rounding of an fp32 computation:
    assert_ulps(max_ulp=1.0), at most 1 % of the elements beyond half an ulp.  logits is the fp32 product of two
    values both sides hold exactly, so it is compared bit for bit.  reduction_bounds.py holds the fp32
    restatement of every stage (these functions at T = float32 on the CPU) to the same check against fp64 for
    these seeds (HEAD_SEEDS), in four summation orders: worst 1.0 ulp, at most 0.16 % of a buffer's elements
    beyond half an ulp, the loss scalars equal.  MI355X, over all 107 stage checks of this module: worst 1.0 ulp, at
    most 0.2 % of a buffer beyond half an ulp, every buffer under 100 elements equal.  Then loss[0], dimg and dtxt
    against fp64 autograd of the plain formula at test_clip_head_loss's tolerances."""
    h = _head(dev, (B, K, D))
    check_forward_stages(h, torch.float64)
    assert torch.equal(h["logits"], (_scale(h["ls"]) * h["mm"].float()).half())
    _head_hard(h, h["label"])
    check_hard_stages(h, torch.float64)
    _check_end_to_end(h, soft=False)


@pytest.mark.parametrize("B,K,D", HEAD_SOFT_SHAPES)
def test_clip_head_soft_stages(dev, B, K, D):
    """The soft-label entry point, stage by stage as test_clip_head_stages, soft_ws (the targets q @ txt_n and
    their gradient) included, then end to end against fp64 autograd (test_clip_head_loss_soft's tolerances)."""
    h = _head(dev, (B, K, D), soft=True)
    check_forward_stages(h, torch.float64)
    _head_soft(h, h["q"])
    check_soft_stages(h, torch.float64)
    _check_end_to_end(h, soft=True)


_HEAD_OUT = ("logits", "dmm", "cos_ws", "loss", "dimg_n", "dtxt_n", "dimg", "dtxt")


def test_clip_head_scale_clamp(dev):
    """exp(logit_scale) is clamped at 100: log(200) gives log(100)'s outputs bit for bit (fp32(log 100) lies
    6e-8 above log 100, so its exponential is not below 100), log(50) gives others."""
    outs = {}
    for s in (50.0, 100.0, 200.0):
        h = _head(dev, (8, 38, 512), ls=math.log(s))
        _head_hard(h, h["label"])
        outs[s] = {k: h[k].clone() for k in _HEAD_OUT}
    for k in _HEAD_OUT:
        assert torch.equal(outs[200.0][k], outs[100.0][k]), k
    for k in ("logits", "dmm", "dimg", "dtxt"):
        assert not torch.equal(outs[50.0][k], outs[100.0][k]), k
    assert torch.equal(outs[100.0]["logits"], (100.0 * h["mm"].float()).half())


@pytest.mark.parametrize("labels", HEAD_SHARED_LABELS)
def test_clip_head_shared_classes(dev, labels):
    """dtxt_kernel's per-class loop: three rows (then all rows) on one class, a class no row uses."""
    h = _head(dev, HEAD_SHARED, labels=labels)
    _head_hard(h, h["label"])
    check_hard_stages(h, torch.float64)
    _check_end_to_end(h, soft=False)


def test_clip_head_bad_labels(dev):
    """A label outside [0, K): NaN loss and the non-finite flag, finite gradients; a valid call clears the flag."""
    h = _head(dev, (8, 38, 512))
    bad = h["label"].clone()
    bad[2], bad[5] = -1, 38
    _head_hard(h, bad)
    loss = h["loss"].cpu()
    assert math.isnan(loss[0].item()) and loss[3].item() == 1.0
    assert torch.isfinite(h["dimg"]).all() and torch.isfinite(h["dtxt"]).all()
    _head_hard(h, h["label"])
    loss = h["loss"].cpu()
    assert loss[3].item() == 0.0 and math.isfinite(loss[0].item())


def test_clip_head_batch_limit(dev):
    """B = 65 is refused by both loss entry points before anything is written; B = 64 runs (the hard-label
    B = 64 case is in test_clip_head_stages)."""
    B, K, D = 65, 10, 512
    img, txt, label, q, ls = (t.to(dev) for t in head_inputs(B, K, D, 1))
    h = _head_buffers(dev, B, K, D, fill=SENTINEL)
    h.update(img=img, txt=txt, ls=ls)
    _head_fwd(h)
    outs = ("dmm", "cos_ws", "loss", "dimg_n", "dtxt_n", "dimg", "dtxt", "soft_ws")
    with pytest.raises(_lib.MapfedError):
        _head_hard(h, label)
    with pytest.raises(_lib.MapfedError):
        _head_soft(h, q)
    torch.cuda.synchronize()
    for k in outs:
        assert (h[k] == SENTINEL).all(), k
    h64 = _head(dev, HEAD_SOFT_B64, soft=True)
    _head_soft(h64, h64["q"])
    check_soft_stages(h64, torch.float64)
    _check_end_to_end(h64, soft=True)


def test_clip_head_zero_row(dev):
    """A zero image row: its norm clamps to 1e-8, its img_n and logits rows are zero, the loss is finite."""
    h = _head(dev, HEAD_ZERO_ROW, zero_row=1)
    label, ls = h["label"], h["ls"]
    assert h["norms"][1].item() == float(np.float32(1e-8))
    assert (h["img_n"][1] == 0).all() and (h["logits"][1] == 0).all() and (h["mm"][1] == 0).all()
    check_forward_stages(h, torch.float64)
    _head_hard(h, label)
    loss = h["loss"].cpu()
    assert math.isfinite(loss[0].item()) and loss[3].item() == 0.0
    r = ref_loss_hard(h["logits"], h["img_n"], h["txt_n"], label, _scale(ls), torch.float64)
    assert_ulps(h["loss"][:3], r["loss"], 1.0, what="loss with a zero row")


@pytest.mark.parametrize("K", [1000, 1])
def test_argmax_correct_wide_and_single(dev, K):
    """argmax_correct on 17 rows (row 16 wraps onto wave 0): at K = 1000 a tie 64 apart (one lane's first and
    second element), a NaN at a high index beside a larger finite value at a low one; K = 1; acc summed over
    two calls."""
    B = 17
    g = torch.Generator().manual_seed(K)
    logits = torch.randn(B, K, generator=g).half()
    if K > 1:
        logits[3, 5] = logits[3, 69] = 50.0     # the same lane's k = 5 and k = 69: the first stays
        logits[16, 69] = logits[16, 5] = 40.0
        logits[4, 2] = 60.0
        logits[4, 901] = float("nan")           # NaN is the maximum (torch.argmax)
        logits[7, 937] = logits[7, 999] = float("nan")
    ref = logits.float().argmax(1)
    if K > 1:
        assert ref[3].item() == 5 and ref[16].item() == 5 and ref[4].item() == 901 and ref[7].item() == 937
    label = torch.randint(0, K, (B,), generator=g)
    label[:6] = ref[:6]
    logits, label = logits.to(dev), label.to(dev)
    pred = torch.full((B,), -5, dtype=torch.int64, device=dev)
    acc = torch.zeros(2, device=dev)
    ops.argmax_correct(logits, label, pred, acc)
    assert torch.equal(pred.cpu(), ref)
    hits = (ref == label.cpu()).sum().item()
    assert acc.tolist() == [hits, B]
    ops.argmax_correct(logits, label, pred, acc)
    assert acc.tolist() == [2 * hits, 2 * B]


# ------------------------------------------------------------------------------------------ gradient-norm clip

CHUNK_DTYPE = np.dtype([("seg", np.int32), ("is16", np.int32), ("s", np.int64), ("e", np.int64)])

# |out[0] - total64| <= CLIP_F32_BOUND * total64 for a table of fp32 segments only.  reduction_bounds.py (fp32
# restatement of sumsq_chunks_kernel's thread / wave / block grouping and of clip_coef_kernel's segmented scan and
# carry, vs fp64, the all-fp32 long table at both scalings and its 1024 / 1025-chunk cuts): worst 1.08e-7; 4x margin.
# The same restatement of the mixed table: at most 9.5e-8, no fp16 segment norm rounded the other way.
# MI355X: 1.07e-7 (all-fp32) and 9.4e-8 (mixed), the restatement's totals digit for digit.
CLIP_F32_BOUND = 4 * 1.08e-7


def clip_table(ce, all32=False, cut=None):
    """The long ragged chunk table: (segments [(id, is16, start, end)], chunk records, n16, n32).  In order: an
    fp16 segment of 1023 full chunks and a 5-element one (tile 0 of clip_coef_kernel exactly); 600 fp32 segments
    of 1..300 elements end to end; an fp32 segment of 1100 chunks from an odd element (crosses the 2048 tile
    boundary); 30 fp16 segments of 3..20 elements at odd starts; an fp16 segment of two chunks.  all32: the same
    structure with every segment in the fp32 buffer.  cut: keep the first `cut` chunks."""
    rng = np.random.RandomState(12)
    pos = {0: 0, 1: 0}  # next free element of the fp32 / fp16 buffer
    segs = []

    def add(is16, n, odd=False):
        buf = 0 if all32 else is16
        if odd and pos[buf] % 2 == 0:
            pos[buf] += 1
        segs.append((len(segs), buf, pos[buf], pos[buf] + n))
        pos[buf] += n

    add(1, 1023 * ce + 5)
    for n in rng.randint(1, 301, size=600):
        add(0, int(n))
    add(0, 1099 * ce + 77, odd=True)
    for n in rng.randint(3, 21, size=30):
        add(1, int(n), odd=True)
    add(1, ce + 100)
    chunks = [(sid, is16, s, min(e, s + ce)) for sid, is16, a, e in segs for s in range(a, e, ce)]
    if cut is not None:
        chunks = chunks[:cut]
    arr = np.array(chunks, dtype=CHUNK_DTYPE)
    # 8-element multiples so that optimizer_step takes its fused 8-wide SGD launch
    return segs, arr, (pos[1] + 7) // 8 * 8, (pos[0] + 7) // 8 * 8


@functools.lru_cache(maxsize=2)
def _clip_base(n16, n32):
    g = torch.Generator().manual_seed(21)
    return torch.randn(n16, generator=g), torch.randn(n32, generator=g)


def clip_grads(n16, n32, scale):
    """Host gradients of standard deviation `scale` (the unit-variance draw is made once and left unchanged)."""
    b16, b32 = _clip_base(n16, n32)
    return (b16 * scale).half(), b32 * scale


def clip_ref64(arr, g16, g32, max_norm=1.0):
    """fp64 on the host: per-segment norm (an fp16 segment's rounded to fp16), total, coefficient, and the
    fp16 segments' share sum_s norm_s^2 2^-11 / total of the total (see test_clip_grad_norm_long_table)."""
    a16, a32 = g16.double().numpy(), g32.double().numpy()
    ss, is16 = {}, {}
    for sid, h, s, e in arr.tolist():
        v = (a16 if h else a32)[s:e]
        ss[sid] = ss.get(sid, 0.0) + float(np.dot(v, v))
        is16[sid] = h
    tot2, share = 0.0, 0.0
    for sid, v in ss.items():
        n = math.sqrt(v)
        if is16[sid]:
            n = float(np.float16(n))
            share += n * n * 2.0 ** -11
        tot2 += n * n
    total = math.sqrt(tot2)
    return total, min(1.0, max_norm / (total + 1e-6)), share / total


def _clip_run(dev, arr, g16, g32):
    chunks = torch.from_numpy(arr.view(np.uint8)).to(dev)
    part = torch.full((len(arr),), float("nan"), device=dev)
    out = torch.full((3,), float("nan"), device=dev)
    ops.clip_grad_norm(g16, g32, chunks, len(arr), 1.0, part, out)
    return chunks, part, out


def _check_clip(out, ref, bound, what):
    total, coef, _ = ref
    o = out.cpu().double().tolist()
    print(f"{what}: total {o[0]:.9g} vs {total:.9g} (rel err {abs(o[0] - total) / total:.3e}, bound {bound:.3e}), "
          f"coef {o[1]:.9g} vs {coef:.9g}")
    assert o[2] == 1.0
    assert abs(o[0] - total) <= bound * total, what
    if coef == 1.0:
        assert o[1] == 1.0, what
    else:  # coef = 1 / (total + 1e-6): the total's relative error plus the fp32 add and divide
        assert abs(o[1] - coef) <= (bound + 2.0 ** -22) * coef, what


@pytest.mark.parametrize("all32", [False, True])
@pytest.mark.parametrize("cut", [None, 1024, 1025])
def test_clip_grad_norm_long_table(dev, cut, all32):
    """clip_grad_norm over a long ragged chunk table (clip_table), whole and cut to 1024 and 1025 chunks, against
    fp64 on the host, once scaled to a total norm above max_norm = 1 (clipped) and once below (coef exactly 1).
    Bound on out[0]: an fp16 segment's norm is rounded to fp16, and the kernel may round the other way than fp64
    does, which moves that norm by one fp16 ulp: relative 2^-11 on that segment's share norm_s^2 / total of the
    total; on top of it CLIP_F32_BOUND (see there), which alone bounds the all-fp32 table.  An inf in one gradient
    clears out[2]."""
    ce = ops.optim_chunk_elems()
    segs, arr, n16, n32 = clip_table(ce, all32, cut)
    assert len(arr) == (cut or len(arr)) and (cut or len(arr) > 2048)
    for scale in (1e-3, 1e-4):
        g16h, g32h = clip_grads(n16, n32, scale)
        ref = clip_ref64(arr, g16h, g32h)
        assert (ref[1] < 1.0) == (scale == 1e-3)
        g16, g32 = g16h.to(dev), g32h.to(dev)
        _, part, out = _clip_run(dev, arr, g16, g32)
        assert torch.isfinite(part).all()
        _check_clip(out, ref, CLIP_F32_BOUND + ref[2] / ref[0], f"cut={cut} all32={all32} scale={scale}")
    sid, is16, s, e = arr[len(arr) - 1].tolist()
    (g16 if is16 else g32)[e - 1] = float("inf")
    _, _, out = _clip_run(dev, arr, g16, g32)
    assert out[2].item() == 0.0


def test_optimizer_step_long_table_matches_unfused(dev):
    """optimizer_step with the long table: out[0], out[1] and p, g and the momentum buffer after it equal
    clip_grad_norm + two sgd_step calls bit for bit (clipped: every gradient is rescaled)."""
    ce = ops.optim_chunk_elems()
    segs, arr, n16, n32 = clip_table(ce)
    g16h, g32h = clip_grads(n16, n32, 1e-3)
    gp = torch.Generator().manual_seed(22)
    p16h, p32h = torch.randn(n16, generator=gp).half(), torch.randn(n32, generator=gp)
    hyper0 = torch.tensor([0.01, 0.9, 5e-4, 1.0, 0.0], device=dev)
    res = []
    for fused in (False, True):
        p16, g16, p32, g32 = p16h.to(dev), g16h.to(dev), p32h.to(dev), g32h.to(dev)
        b16, b32 = torch.zeros_like(p16), torch.zeros_like(p32)
        chunks = torch.from_numpy(arr.view(np.uint8)).to(dev)
        part = torch.empty(len(arr), device=dev)
        out = torch.empty(3, device=dev)
        hyper = hyper0.clone()
        if fused:
            ops.optimizer_step(p16, g16, b16, p32, g32, b32, chunks, len(arr), 1.0, part, out, hyper,
                               torch.zeros(1, device=dev))
        else:
            ops.clip_grad_norm(g16, g32, chunks, len(arr), 1.0, part, out)
            ops.sgd_step(p16, g16, b16, out, hyper)
            ops.sgd_step(p32, g32, b32, out, hyper)
        res.append((out, part, p16, g16, b16, p32, g32, b32))
    assert res[0][0][1].item() < 1.0
    assert not torch.equal(res[0][3], g16h.to(dev))
    for a, b in zip(*res):
        assert torch.equal(a, b)
